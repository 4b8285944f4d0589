"""rpo_layernorm_bwd requests every column chunk's x, gamma, dy slabs and dres before it uses any of them (csrc/norm.hip,
DESIGN.md 11f).  The order of the loads must not show in the results: every register count the launcher picks (2, 3, 4, 8
float4 per lane, d up to 2048), every slab count around the four that are fetched unconditionally (clamped index, masked
add) and the loop behind them, strided operands, with and without dres / the cast copy."""
import pytest
import torch

from rpo_amd import ops as o

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
ROWS = 50                                        # no multiple of anything; more than one workgroup
EPS = 1e-5


def _ref64(dy, x, gamma, dres):
    """dres + rstd * (g - mean(g) - xhat * mean(g * xhat)), g = dy * gamma, in float64."""
    x, g = x.double(), dy.double() * gamma.double()
    xc = x - x.mean(1, keepdim=True)
    rstd = (xc.pow(2).mean(1, keepdim=True) + EPS).rsqrt()
    xh = xc * rstd
    out = rstd * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    return out if dres is None else out + dres.double()


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(11)
    out = {}
    for d in (512, 768, 1024, 2048):
        wide = torch.randn(ROWS, d + 8, generator=g).to(DEV)                     # (row stride d + 8: strided x)
        out[d] = dict(x=(2.0 * wide + 0.3)[:, :d], gamma=(1 + 0.1 * torch.randn(d, generator=g)).to(DEV),
                      dres=torch.randn(ROWS, d, generator=g).to(DEV), slabs=torch.randn(6, ROWS, d, generator=g).to(DEV))
    return out


@pytest.mark.parametrize("d", [512, 768, 1024, 2048])
def test_slab_counts_against_float64(data, d):
    """Bound: the kernel keeps fp32 throughout; a value passes through at most S <= 6 slab adds, d / 64 <= 32 adds per lane
    and 6 exchange steps per reduction, and about ten further operations: under 60 roundings of 2^-24 = 3.6e-6 relative to
    the largest intermediate, which for these unit-scale inputs stays within 3x of max |ref|.  So 1e-5 * max |ref|."""
    t = data[d]
    for S in (1, 2, 3, 4, 5, 6):
        buf = torch.full((8, ROWS, d), float("nan"), device=DEV)                 # slabs past S are NaN: never read
        buf[:S] = t["slabs"][:S]
        dy = buf[0] if S == 1 else buf[:S]
        for dres in (t["dres"], None):
            dx = torch.full((ROWS, d), float("nan"), device=DEV)
            o.layernorm_bwd(dy, t["x"], t["gamma"], dres, dx, None)
            ref = _ref64(t["slabs"][:S].double().sum(0), t["x"], t["gamma"], dres)
            err = float((dx.double() - ref).abs().max() / ref.abs().max())
            print(f"d={d} S={S} dres={dres is not None}: rel err {err:.2e}")
            assert err <= 1e-5


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("d", [512, 768, 1024, 2048])
def test_zero_slabs_and_cast_copy_are_exact(data, d, mode):
    """Adding slabs of zeros changes no bit (fma(1, 0, t) = t; t + 0 = t) whichever path fetches them, the cast copy is dx
    rounded to nearest even, and a 16-bit dy gives the bits of the same values passed as fp32."""
    t = data[d]
    dy16 = t["slabs"][0].to(DT[mode])

    def run(dy):
        dx = torch.full((ROWS, d), float("nan"), device=DEV)
        dxc = torch.full((ROWS, d), float("nan"), device=DEV, dtype=DT[mode])
        o.layernorm_bwd(dy, t["x"], t["gamma"], t["dres"], dx, dxc)
        return dx, dxc
    dx0, dxc0 = run(dy16)
    assert torch.isfinite(dx0).all() and torch.equal(dxc0, dx0.to(DT[mode]))
    for S in (1, 2, 4, 5, 6):
        buf = torch.zeros(S, ROWS, d, device=DEV)
        buf[0] = dy16.float()
        dx, dxc = run(buf[0] if S == 1 else buf)
        assert torch.equal(dx, dx0) and torch.equal(dxc, dxc0), f"S={S}"
