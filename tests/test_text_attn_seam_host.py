"""What tests/test_gpu_text_attn_seam.py covers, proved on the CPU from its own case table and dispatch model, and the
float64 oracle it leans on checked at the key limit (tests/test_oracle_rows.py stops at 71 keys)."""
import math

import torch

_DEVICE_UP_BEFORE = torch.cuda.is_initialized()
import test_gpu_text_attn_seam as S  # noqa: E402
_DEVICE_UP_AFTER = torch.cuda.is_initialized()
from oracle import rows_oracle as R  # noqa: E402


def _kernels(aligned=True):
    """{(kernel, query tiles)} over the table and the three storage modes"""
    return {(S.expected_kernel(mode, rows, Lmax, aligned), (rows + 31) // 32)
            for Lmax, rows, _ in S.CASES.values() for mode in S.MODES}


def test_importing_the_gpu_module_left_the_device_alone():
    assert _DEVICE_UP_AFTER == _DEVICE_UP_BEFORE


def test_the_table_holds_the_cases_of_the_issue():
    want = {"L32_r45": (32, 45), "L33_r44": (33, 44), "L64_r13": (64, 13), "L65_r12": (65, 12), "L77_r32": (77, 32),
            "L77_r33": (77, 33), "L77_r64": (77, 64), "L77_r65": (77, 65), "L96_r24": (96, 24), "L97_r24": (97, 24),
            "L126_r5": (126, 5), "L127_r5": (127, 5), "L128_r24": (128, 24), "L128_r1": (128, 1)}
    assert len(set(S.IDS)) == len(S.IDS)
    for cid, (Lmax, rows) in want.items():
        assert S.CASES[cid][:2] == (Lmax, rows), cid
    assert set(S.SHARED_IDS) == {"L33_r44", "L77_r65", "L96_r24", "L97_r24", "L128_r24"}
    assert set(S.SHARP) == {(96, 24, "bf16"), (96, 24, "f16"), (97, 24, "bf16"), (97, 24, "f16"), (128, 24, "f32"),
                            (128, 24, "bf16"), (128, 24, "f16"), (33, 44, "bf16"), (33, 44, "f16")}
    assert S.CAUSAL_LMAX == (96, 127, 128)


def test_every_kernel_with_one_and_with_two_query_tiles():
    got = _kernels()
    for kern in ("wave1", "wave2", "wave3"):
        assert (kern, 1) in got and (kern, 2) in got, f"{kern}: {sorted(t for k, t in got if k == kern)} query tiles only"
    assert any(k == "valu" for k, _ in got)
    # the wave kernel's row limit on both sides, and its one-live-row second tile
    rows_16bit = {rows for Lmax, rows, _ in S.CASES.values() if Lmax <= 96}
    assert {32, 33, 64, 65} <= rows_16bit


def test_the_valu_kernel_is_reached_by_dtype_rows_keys_and_alignment():
    reasons = set()
    for Lmax, rows, _ in S.CASES.values():
        if S.expected_kernel("bf16", rows, Lmax, True) != "valu":
            assert S.expected_kernel("f16", rows, Lmax, True) == S.expected_kernel("bf16", rows, Lmax, True)
            assert S.expected_kernel("f32", rows, Lmax, True) == "valu"
            reasons.add("dtype")
        elif rows > 64 and Lmax <= 96:
            reasons.add("rows")
        elif rows <= 64 and Lmax > 96:
            reasons.add("Lmax")
    # alignment: the views of test 1 keep a 16-bit call on its kernel, every variant of test 2 but the first leaves it
    assert S.views_aligned("pitched", False) and S.views_aligned("pitched", True)
    assert S.views_aligned("aligned", False) and S.views_aligned("aligned", True)
    assert not any(S.views_aligned(v, False) for v in S.FWD_UNALIGNED)
    assert not any(S.views_aligned(v, True) for v in S.BWD_UNALIGNED)
    for cid in S.UNALIGNED_IDS:
        Lmax, rows, _ = S.CASES[cid]
        for mode in ("bf16", "f16"):
            assert S.expected_kernel(mode, rows, Lmax, True).startswith("wave")
            assert S.expected_kernel(mode, rows, Lmax, False) == "valu"
    assert {S.expected_kernel("bf16", *S.CASES[cid][1::-1], True) for cid in S.UNALIGNED_IDS} == {"wave1", "wave2", "wave3"}
    reasons.add("alignment")
    assert reasons == {"dtype", "rows", "Lmax", "alignment"}


def test_key_counts_on_both_sides_of_every_switch():
    keys = {Lmax for Lmax, _, _ in S.CASES.values()}
    assert {32, 33, 64, 65, 96, 97, 128} <= keys
    lds = sorted(S.valu_lds_bytes(L) for L in keys)
    assert max(b for b in lds if b <= 65536) == S.valu_lds_bytes(126) == 65520
    assert min(b for b in lds if b > 65536) == S.valu_lds_bytes(127) == 66040
    for Lmax, Kr, mode in S.SHARP:
        lens = S.sharp_lens(Lmax)
        assert max(lens) == Lmax and 1 in lens and {e for e in (33, 65) if e <= Lmax} <= set(lens)
    assert {S.expected_kernel(m, Kr, L, True) for L, Kr, m in S.SHARP} == {"wave2", "wave3", "valu"}


def test_every_class_list_holds_the_limit_one_key_the_tile_edges_and_a_len_past_the_limit():
    for cid, (Lmax, rows, lens) in S.CASES.items():
        assert Lmax in lens and 1 in lens, cid
        assert {e for e in S.EDGES if e <= Lmax} <= set(lens), cid
        assert lens.count(Lmax + 5) == 1 and max(lens) == Lmax + 5, cid
        assert len(lens) <= 12 and min(lens) >= 1, cid


def test_rows_oracle_at_128_keys_against_float64_autograd():
    """attn_rows_fwd / attn_rows_bwd at the key limit, 1e-12 relative"""
    H, N, rows = 2, 128, 5
    g = torch.Generator().manual_seed(7)
    q = (torch.randn(rows, 64 * H, generator=g, dtype=torch.float64) * 1.5).requires_grad_()
    k, v, da = (torch.randn(n, 64 * H, generator=g, dtype=torch.float64) for n in (N, N, rows))
    heads = lambda x: x.reshape(x.shape[0], H, 64).transpose(0, 1)
    p = torch.softmax(heads(q) @ heads(k).transpose(1, 2) / math.sqrt(64), dim=-1)
    out = (p @ heads(v)).transpose(0, 1).reshape(rows, 64 * H)
    dq, = torch.autograd.grad((out * da).sum(), q)
    for got, ref in ((R.attn_rows_fwd(q.detach(), k, v, H), out.detach()), (R.attn_rows_bwd(q.detach(), k, v, da, H), dq)):
        assert got.dtype == torch.float64
        assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
