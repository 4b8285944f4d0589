"""rpo_amd: CLIP prompt-learning trainers on hand-written HIP for gfx950.  The trainers live in their own modules;
`rpo_amd.LPSweep`, `rpo_amd.CoCoOpMulti` and `rpo_amd.CoOpSweep` resolve on first use, so importing the package stays as
cheap as it was."""
__all__ = ["LPSweep", "CoCoOpMulti", "CoOpSweep"]


def __getattr__(name):
    if name == "LPSweep":
        from .lp_sweep import LPSweep
        return LPSweep
    if name == "CoCoOpMulti":
        from .coop_multi import CoCoOpMulti
        return CoCoOpMulti
    if name == "CoOpSweep":
        from .coop_sweep import CoOpSweep
        return CoOpSweep
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
