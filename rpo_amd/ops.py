"""Thin torch-tensor front-end of the C ABI (include/rpo_amd.h).

PyTorch is plumbing here: it owns device memory and streams; every function
below only passes ``data_ptr()``s, sizes and the current HIP stream to
librpo_hip.so.  No computation happens in torch, and there is no fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import (EPI_BIAS, EPI_BIAS_QGELU, EPI_BIAS_RESID, EPI_NONE, EPI_PATCH, EPI_QGELU_BWD, RPO_BF16,
                   RPO_F16, RPO_F32, GemmArgs, check)

LN_EPS = 1e-5


def dtype_code(t: torch.dtype) -> int:
    if t == torch.float32:
        return RPO_F32
    if t == torch.bfloat16:
        return RPO_BF16
    if t == torch.float16:
        return RPO_F16
    raise TypeError(f"unsupported dtype {t}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _ld(t: torch.Tensor) -> int:
    assert t.dim() == 2 and t.stride(1) == 1, "row-major 2-D view required"
    return t.stride(0)


def version() -> int:
    return _lib.load().rpo_version()


def gemm_args(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, epilogue: int = EPI_NONE,
            bias: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None,
            aux: Optional[torch.Tensor] = None, aux_row0: int = 0, skip_row0: int = -1, skip_col0: int = -1,
            group: int = 0, m_rows: Optional[int] = None, split_k: int = 1, tile_config: int = 0,
            out2: Optional[torch.Tensor] = None, ln_stats: Optional[torch.Tensor] = None,
            ln_colsum: Optional[torch.Tensor] = None, ln_eps: float = LN_EPS,
            row_units: Optional[tuple] = None, ln_group: int = 0,
            prefetch: Optional[torch.Tensor] = None, resid_hi: Optional[torch.Tensor] = None,
            resid_lo: Optional[torch.Tensor] = None, out_lo: Optional[torch.Tensor] = None, c_row0: int = 0) -> GemmArgs:
    """The rpo_gemm_args of out = a @ w.T with a fused epilogue.  For EPI_PATCH ``out`` is the token matrix
    (more rows than ``a``); ``m_rows`` overrides M otherwise taken from ``a``.  With
    ``split_k`` = S > 1, ``out`` is [S, M, N] fp32 slabs to be summed by the consumer.
    LayerNorm fold: a BIAS_RESID call may also leave ``out2`` (act-dtype copy of its result) and ``ln_stats``
    ([M, N/64, 2] partial row statistics); an LN_BIAS / LN_BIAS_QGELU call reads such ``ln_stats`` for its A rows
    together with ``ln_colsum`` (see include/rpo_amd.h)."""
    M = a.shape[0] if m_rows is None else m_rows
    N, K = w.shape
    assert a.shape[1] == K and a.dtype == w.dtype
    split_stride = 0
    if split_k > 1:
        assert out.dim() == 3 and out.shape[0] == split_k and out.stride(2) == 1
        split_stride, ldc = out.stride(0), out.stride(1)
    else:
        ldc = _ld(out)
    args = GemmArgs(A=a.data_ptr(), lda=_ld(a), W=w.data_ptr(), ldw=_ld(w), C=out.data_ptr(), ldc=ldc,
                    M=M, N=N, K=K, in_dtype=dtype_code(a.dtype), out_dtype=dtype_code(out.dtype),
                    epilogue=epilogue, bias=_p(bias), resid=_p(resid), ldr=0 if resid is None else _ld(resid),
                    aux=_p(aux), ldaux=0 if aux is None else _ld(aux), aux_row0=aux_row0,
                    skip_row0=skip_row0, skip_col0=skip_col0, group=group, split_k=split_k,
                    split_stride=split_stride, tile_config=tile_config,
                    out2=_p(out2), ldout2=0 if out2 is None else _ld(out2), ln_stats=_p(ln_stats),
                    ln_colsum=_p(ln_colsum), ln_eps=ln_eps)
    args.ln_group = ln_group
    if resid_hi is not None:                # residual stream as 16-bit hi / lo halves (include/rpo_amd.h)
        assert resid_hi.dtype == a.dtype and (resid_lo is None or (resid_lo.dtype == a.dtype and _ld(resid_hi) == _ld(resid_lo)))
        args.resid_hi, args.resid_lo, args.ldr16 = resid_hi.data_ptr(), _p(resid_lo), _ld(resid_hi)
    if out_lo is not None:
        assert out2 is not None and out_lo.dtype == out2.dtype and _ld(out_lo) == _ld(out2)
        args.out_lo = out_lo.data_ptr()
    args.c_row0 = c_row0
    if prefetch is not None:                # hint: what the next launch reads first (include/rpo_amd.h)
        assert prefetch.is_contiguous()
        args.prefetch, args.prefetch_bytes = prefetch.data_ptr(), prefetch.numel() * prefetch.element_size()
    if aux is not None and aux.dtype != torch.float32:      # 16-bit aux: holds d quickgelu / du (include/rpo_amd.h)
        args.aux_dtype = dtype_code(aux.dtype)
    if row_units is not None:               # (rows per unit in segment 0, rows per unit in segment 1, first row of segment 1)
        args.seg_rows0, args.seg_rows1, args.seg1_row0 = row_units
    if ln_stats is not None:
        rows = a.shape[0] if epilogue in (_lib.EPI_LN_BIAS, _lib.EPI_LN_BIAS_QGELU) else M
        cols = K if epilogue in (_lib.EPI_LN_BIAS, _lib.EPI_LN_BIAS_QGELU) else N
        assert ln_stats.dtype == torch.float32 and ln_stats.is_contiguous() and ln_stats.numel() >= rows * (cols // (ln_group or 64)) * 2
    return args


def gemm_nt(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, epilogue: int = EPI_NONE, **kw) -> torch.Tensor:
    """out = a @ w.T with a fused epilogue (rpo_gemm_nt); keyword arguments as `gemm_args`."""
    args = gemm_args(a, w, out, epilogue, **kw)
    check(_lib.load().rpo_gemm_nt(C.byref(args), _stream()), "rpo_gemm_nt")
    return out


class PackedWeight:
    """A frozen [N, K] weight in rpo_gemm_ws's fragment-major order (rpo_gemm_ws_pack): what `gemm_ws` takes as W."""
    __slots__ = ("data", "N", "K", "dtype")

    def __init__(self, data: torch.Tensor, N: int, K: int):
        self.data, self.N, self.K, self.dtype = data, N, K, data.dtype

    # the prefetch hint names its bytes (ops.gemm_args: prefetch=...)
    def is_contiguous(self) -> bool:
        return True

    def data_ptr(self) -> int:
        return self.data.data_ptr()

    def numel(self) -> int:
        return self.data.numel()

    def element_size(self) -> int:
        return self.data.element_size()


def gemm_ws_pack(w: torch.Tensor) -> PackedWeight:
    """Fragment-major copy of a row-major 16-bit [N, K] weight (N % 32 == 0, K % 64 == 0)."""
    N, K = w.shape
    out = torch.empty(N * K, dtype=w.dtype, device=w.device)
    check(_lib.load().rpo_gemm_ws_pack(w.data_ptr(), _ld(w), out.data_ptr(), N, K, dtype_code(w.dtype), _stream()),
          "rpo_gemm_ws_pack")
    return PackedWeight(out, N, K)


class _WView:
    """stand-in for the weight tensor in gemm_args (shape / dtype / pointer of the packed copy)"""
    def __init__(self, pw: PackedWeight):
        self.shape, self.dtype, self._pw = (pw.N, pw.K), pw.dtype, pw

    def data_ptr(self) -> int:
        return self._pw.data_ptr()

    def dim(self) -> int:
        return 2

    def stride(self, i: int) -> int:
        return (self._pw.K, 1)[i]


def gemm_ws(a: torch.Tensor, w: PackedWeight, out: torch.Tensor, epilogue: int = EPI_NONE, **kw) -> torch.Tensor:
    """out = a @ W.T with a fused epilogue for the prompt rows (rpo_gemm_ws): `w` is the packed copy of W; keyword
    arguments as `gemm_args`."""
    args = gemm_args(a, _WView(w), out, epilogue, **kw)
    check(_lib.load().rpo_gemm_ws(C.byref(args), _stream()), "rpo_gemm_ws")
    return out


def gemm_ws_try(a: torch.Tensor, w: PackedWeight, out: torch.Tensor, epilogue: int = EPI_NONE, **kw) -> bool:
    """`gemm_ws`, but a problem the kernel does not take (RPO_E_SHAPE: nothing was enqueued) returns False instead of
    raising, so that the caller can issue rpo_gemm_nt on the row-major weight; every other error still raises."""
    args = gemm_args(a, _WView(w), out, epilogue, **kw)
    rc = int(_lib.load().rpo_gemm_ws(C.byref(args), _stream()))
    if rc == _lib.E_SHAPE:
        return False
    check(rc, "rpo_gemm_ws")
    return True


def gemm_ws_ok(M: int, N: int, K: int, dtype: torch.dtype, out_dtype: torch.dtype, epilogue: int, split_k: int = 1,
               stats: bool = False) -> bool:
    """Does rpo_gemm_ws take this problem (rpo_gemm_ws_ok)?"""
    if dtype == torch.float32:
        return False
    args = GemmArgs(M=M, N=N, K=K, lda=K, ldw=K, ldc=N, in_dtype=dtype_code(dtype), out_dtype=dtype_code(out_dtype),
                    epilogue=epilogue, split_k=split_k, split_stride=M * N, skip_row0=-1, skip_col0=-1)
    if stats:
        args.ln_stats = 4096
    return int(_lib.load().rpo_gemm_ws_ok(C.byref(args))) == 1


def gemm_nt_pair(g0: dict, g1: dict) -> None:
    """Two small-M GEMMs of the same kind in ONE launch (rpo_gemm_nt_pair): g0 / g1 are the keyword arguments of
    `gemm_nt` (a, w, out, epilogue, ...) of the two problems."""
    a0, a1 = gemm_args(**g0), gemm_args(**g1)
    check(_lib.experimental().rpo_gemm_nt_pair(C.byref(a0), C.byref(a1), _stream()), "rpo_gemm_nt_pair")


def mlp_fused(fc: dict, proj: dict, counters: torch.Tensor, safe: bool = False) -> bool:
    """c_fc -> c_proj in ONE launch (rpo_mlp_fused): fc / proj are the keyword arguments of the two `gemm_nt` calls it
    stands for (a, w, out, epilogue, ...).  Returns False where the kernel does not apply (RPO_E_SHAPE): the caller then
    issues the two calls."""
    a0, a1 = gemm_args(**fc), gemm_args(**proj)
    assert counters.dtype == torch.int32 and counters.is_contiguous()
    rc = _lib.experimental().rpo_mlp_fused(C.byref(a0), C.byref(a1), counters.data_ptr(), int(safe), _stream())
    if rc == -2:                                     # RPO_E_SHAPE
        return False
    check(rc, "rpo_mlp_fused")
    return True


def gemm_stats_group(M: int, N: int, K: int, dtype: torch.dtype, row_units: Optional[tuple]) -> int:
    """Columns per partial row statistic a BIAS_RESID producer [M, K] x [N, K]^T -> fp32 writes (rpo_gemm_stats_group)."""
    if dtype == torch.float32:
        return 64
    args = GemmArgs(M=M, N=N, K=K, lda=K, ldw=K, ldc=N, in_dtype=dtype_code(dtype), out_dtype=_lib.RPO_F32,
                    epilogue=_lib.EPI_BIAS_RESID, split_k=1)
    if row_units is not None:
        args.seg_rows0, args.seg_rows1, args.seg1_row0 = row_units
    g = int(_lib.load().rpo_gemm_stats_group(C.byref(args)))
    if g < 0:
        check(g, "rpo_gemm_stats_group")
    return g


def gemm_nt_plan(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, epilogue: int = EPI_NONE, **kw) -> int:
    """The tile_config value that forces the kernel `gemm_nt` would run with these arguments (> 0), or the negative RPO_E_*
    it would return (rpo_gemm_nt_plan).  Nothing is launched."""
    args = gemm_args(a, w, out, epilogue, **kw)
    return int(_lib.load().rpo_gemm_nt_plan(C.byref(args)))


def gemm_ws_plan(a: torch.Tensor, w: PackedWeight, out: torch.Tensor, epilogue: int = EPI_NONE, **kw) -> int:
    """`gemm_nt_plan` for `gemm_ws`: its geometry as the tile_config code 100 * MT + 10 * NT (> 0), or the negative RPO_E_*
    it would return (rpo_gemm_ws_plan).  Nothing is launched."""
    args = gemm_args(a, _WView(w), out, epilogue, **kw)
    return int(_lib.load().rpo_gemm_ws_plan(C.byref(args)))


def gemm_hilo_ok(M: int, N: int, K: int, dtype: torch.dtype, row_units: Optional[tuple], ln_group: int = 0) -> bool:
    """Would a BIAS_RESID GEMM of these shapes run on a kernel that implements the hi / lo residual stream
    (rpo_gemm_hilo_ok)?"""
    if dtype == torch.float32:
        return False
    args = GemmArgs(M=M, N=N, K=K, lda=K, ldw=K, ldc=N, in_dtype=dtype_code(dtype), out_dtype=_lib.RPO_F32,
                    epilogue=_lib.EPI_BIAS_RESID, split_k=1)
    args.ln_group = ln_group
    if row_units is not None:
        args.seg_rows0, args.seg_rows1, args.seg1_row0 = row_units
    return int(_lib.load().rpo_gemm_hilo_ok(C.byref(args))) == 1


def layernorm_fwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, y: torch.Tensor,
                  eps: float = LN_EPS) -> torch.Tensor:
    assert x.dtype == torch.float32
    check(_lib.load().rpo_layernorm_fwd(x.data_ptr(), _ld(x), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(),
                                        _ld(y), dtype_code(y.dtype), x.shape[0], x.shape[1], eps, _stream()),
          "rpo_layernorm_fwd")
    return y


def layernorm_bwd(dy: torch.Tensor, x: torch.Tensor, gamma: torch.Tensor, dres: Optional[torch.Tensor],
                  dx: torch.Tensor, dx_cast: Optional[torch.Tensor] = None, eps: float = LN_EPS) -> torch.Tensor:
    assert x.dtype == torch.float32 and dx.dtype == torch.float32
    splits, split_stride = 1, 0
    if dy.dim() == 3:                       # [S, rows, d] split-K slabs
        splits, split_stride, lddy = dy.shape[0], dy.stride(0), dy.stride(1)
    else:
        lddy = _ld(dy)
    check(_lib.load().rpo_layernorm_bwd(
        dy.data_ptr(), dtype_code(dy.dtype), lddy, x.data_ptr(), _ld(x), gamma.data_ptr(),
        _p(dres), 0 if dres is None else _ld(dres), dx.data_ptr(), _ld(dx), _p(dx_cast),
        RPO_F32 if dx_cast is None else dtype_code(dx_cast.dtype), 0 if dx_cast is None else _ld(dx_cast),
        x.shape[0], x.shape[1], eps, splits, split_stride, _stream()), "rpo_layernorm_bwd")
    return dx


def _ln_bwd_args(dy, x, gamma, dres, dx, dx_cast=None, eps: float = LN_EPS) -> "_lib.LnBwdArgs":
    assert dy.dtype == torch.float32 and x.dtype == torch.float32 and dx.dtype == torch.float32
    splits, split_stride = 1, 0
    if dy.dim() == 3:
        splits, split_stride, lddy = dy.shape[0], dy.stride(0), dy.stride(1)
    else:
        lddy = _ld(dy)
    return _lib.LnBwdArgs(dy=dy.data_ptr(), lddy=lddy, x=x.data_ptr(), ldx=_ld(x), gamma=gamma.data_ptr(),
                          dres=_p(dres), lddres=0 if dres is None else _ld(dres), dx=dx.data_ptr(), lddx=_ld(dx),
                          dx_cast=_p(dx_cast), cast_dtype=RPO_F32 if dx_cast is None else dtype_code(dx_cast.dtype),
                          ldcast=0 if dx_cast is None else _ld(dx_cast), rows=x.shape[0], d=x.shape[1], eps=eps,
                          dy_splits=splits, dy_split_stride=split_stride)


def layernorm_bwd_pair(l0: dict, l1: dict) -> None:
    """Two `layernorm_bwd` problems (keyword arguments dy, x, gamma, dres, dx, dx_cast) in ONE launch."""
    a0, a1 = _ln_bwd_args(**l0), _ln_bwd_args(**l1)
    check(_lib.experimental().rpo_layernorm_bwd_pair(C.byref(a0), C.byref(a1), _stream()), "rpo_layernorm_bwd_pair")


def _attn_bwd_args(q_rows, k, v, dx, w_out_t, dq, groups: int, H: int, keys: int, Kp: int, scale: float = 0.125,
                   key_len: Optional[torch.Tensor] = None, key_stride: int = 0) -> "_lib.AttnBwdArgs":
    assert q_rows.dtype == k.dtype == v.dtype == dx.dtype == w_out_t.dtype == dq.dtype and _ld(k) == _ld(v)
    if key_len is not None:
        assert key_len.dtype == torch.int32 and key_len.is_contiguous() and key_len.numel() >= groups
    return _lib.AttnBwdArgs(q_rows=q_rows.data_ptr(), ldq=_ld(q_rows), k=k.data_ptr(), v=v.data_ptr(), ldkv=_ld(k),
                            dx=dx.data_ptr(), lddx=_ld(dx), w_out_t=w_out_t.data_ptr(), ldw=_ld(w_out_t),
                            dq=dq.data_ptr(), lddq=_ld(dq), groups=groups, H=H, keys=keys, Kp=Kp,
                            key_len=_p(key_len), key_stride=key_stride, scale=scale)


def attn_bwd_proj_pair(p0: dict, p1: Optional[dict] = None) -> None:
    """Attention backward of the prompt rows with the d out-proj GEMM folded in, for one or two problems in ONE launch
    (rpo_attn_bwd_proj_pair).  p0 / p1: keyword arguments q_rows, k, v, dx, w_out_t, dq, groups, H, keys, Kp, scale and,
    for per-group key counts (the text tower's K / V cache), key_len (int32 [groups]) + key_stride."""
    a0 = _attn_bwd_args(**p0)
    a1 = None if p1 is None else _attn_bwd_args(**p1)
    check(_lib.experimental().rpo_attn_bwd_proj_pair(C.byref(a0), None if a1 is None else C.byref(a1),
                                             dtype_code(p0["dq"].dtype), _stream()), "rpo_attn_bwd_proj_pair")


def im2col_patches(img: torch.Tensor, out: torch.Tensor, patch: int) -> torch.Tensor:
    B, Cc, H, W = img.shape
    assert Cc == 3 and img.dtype == torch.float32 and img.is_contiguous()
    check(_lib.load().rpo_im2col_patches(img.data_ptr(), out.data_ptr(), dtype_code(out.dtype), _ld(out), B, H, W,
                                         patch, _stream()), "rpo_im2col_patches")
    return out


def img_embed_norm(x_pre, cls, pos0, img_prompt, g_pre, b_pre, x0, g1, b1, h, B: int, N: int, Kp: int,
                   eps: float = LN_EPS, rows: Optional[tuple] = None):
    """img_assemble + ln_pre (-> x0) + the first block's ln_1 (-> h) in one launch.  rows = (row0, row1): those token rows
    only (rpo_img_embed_norm_rows: the frozen rows [0, B*N) do not depend on the prompts)."""
    r0, r1 = (0, B * (N + Kp)) if rows is None else rows
    check(_lib.load().rpo_img_embed_norm_rows(x_pre.data_ptr(), _ld(x_pre), cls.data_ptr(), pos0.data_ptr(), _p(img_prompt),
                                              g_pre.data_ptr(), b_pre.data_ptr(), x0.data_ptr(), _ld(x0), g1.data_ptr(),
                                              b1.data_ptr(), h.data_ptr(), _ld(h), dtype_code(h.dtype), B, N, Kp,
                                              x_pre.shape[1], eps, r0, r1, _stream()), "rpo_img_embed_norm_rows")
    return h


def img_embed_norm_grouped(x_pre, cls, pos0, img_prompt, g_pre, b_pre, x0, g1, b1, h, B: int, N: int, Kp: int,
                           images_per_group: int, eps: float = LN_EPS, rows: Optional[tuple] = None):
    """`img_embed_norm` with one prompt set per group of images: img_prompt [B / images_per_group, Kp, d] (the sets may be
    strided: a column block of a wider parameter buffer) and image b reads set b / images_per_group
    (rpo_img_embed_norm_grouped)."""
    r0, r1 = (0, B * (N + Kp)) if rows is None else rows
    assert tuple(img_prompt.shape) == (B // images_per_group, Kp, x_pre.shape[1]) and img_prompt[0].is_contiguous()
    check(_lib.load().rpo_img_embed_norm_grouped(x_pre.data_ptr(), _ld(x_pre), cls.data_ptr(), pos0.data_ptr(),
                                                 img_prompt.data_ptr(), g_pre.data_ptr(), b_pre.data_ptr(), x0.data_ptr(),
                                                 _ld(x0), g1.data_ptr(), b1.data_ptr(), h.data_ptr(), _ld(h),
                                                 dtype_code(h.dtype), B, N, Kp, x_pre.shape[1], eps, r0, r1,
                                                 images_per_group, img_prompt.stride(0), _stream()),
          "rpo_img_embed_norm_grouped")
    return h


def img_assemble(x: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, img_prompt: torch.Tensor, B: int, N: int,
                 Kp: int) -> torch.Tensor:
    check(_lib.load().rpo_img_assemble(x.data_ptr(), _ld(x), cls.data_ptr(), pos.data_ptr(), img_prompt.data_ptr(),
                                       B, N, Kp, x.shape[1], _stream()), "rpo_img_assemble")
    return x


def broadcast_rows(src: torch.Tensor, dst: torch.Tensor, groups: int) -> torch.Tensor:
    rows, d = src.shape
    assert src.is_contiguous() and dst.shape[0] >= groups * rows
    check(_lib.load().rpo_broadcast_rows(src.data_ptr(), dst.data_ptr(), _ld(dst), groups, rows, d, _stream()),
          "rpo_broadcast_rows")
    return dst


def reduce_groups(src: torch.Tensor, out: torch.Tensor, groups: int) -> torch.Tensor:
    rows, d = out.shape
    assert out.is_contiguous()
    check(_lib.load().rpo_reduce_groups(src.data_ptr(), _ld(src), out.data_ptr(), groups, rows, d, _stream()),
          "rpo_reduce_groups")
    return out


def text_embed(ids: torch.Tensor, table: torch.Tensor, pos: torch.Tensor, out: torch.Tensor, L: int,
               ctx: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[c * L + p] = table[ids[c, p]] + pos[p] (an id < 0: ctx[-1 - id] + pos[p]) for p < L (rpo_text_embed): ids int32
    [n, ld_ids] on the device, table [vocab, d], pos [>= L, d], ctx [n_ctx, d] or None, out [n * L, d], all fp32."""
    n, (vocab, d) = ids.shape[0], table.shape
    assert ids.dtype == torch.int32 and ids.dim() == 2 and ids.stride(1) == 1 and ids.is_cuda
    assert table.dtype == pos.dtype == out.dtype == torch.float32 and table.is_contiguous() and pos.is_contiguous()
    assert out.is_contiguous() and pos.shape[0] >= L and pos.shape[1] == d and out.numel() == n * L * d
    n_ctx = 0 if ctx is None else ctx.shape[0]
    assert ctx is None or (ctx.dtype == torch.float32 and ctx.is_contiguous() and ctx.shape[1] == d)
    check(_lib.load().rpo_text_embed(ids.data_ptr(), ids.stride(0), table.data_ptr(), vocab, pos.data_ptr(), _p(ctx), n_ctx,
                                     out.data_ptr(), n, L, d, _stream()), "rpo_text_embed")
    return out


def broadcast_rows_sets(src: torch.Tensor, dst: torch.Tensor, groups: int) -> torch.Tensor:
    """dst[(s*groups + g)*rows + i] = src[s, i] for src [sets, rows, d], sets possibly strided (rpo_broadcast_rows_sets)."""
    sets, rows, d = src.shape
    assert src[0].is_contiguous() and dst.shape[0] >= sets * groups * rows
    check(_lib.load().rpo_broadcast_rows_sets(src.data_ptr(), src.stride(0), dst.data_ptr(), _ld(dst), sets, groups, rows, d,
                                              _stream()),
          "rpo_broadcast_rows_sets")
    return dst


def reduce_groups_sets(src: torch.Tensor, out: torch.Tensor, groups: int) -> torch.Tensor:
    """out[s, i] = sum_g src[(s*groups + g)*rows + i] for out [sets, rows, d], sets possibly strided (rpo_reduce_groups_sets)."""
    sets, rows, d = out.shape
    assert out[0].is_contiguous() and src.shape[0] >= sets * groups * rows
    check(_lib.load().rpo_reduce_groups_sets(src.data_ptr(), _ld(src), out.data_ptr(), out.stride(0), sets, groups, rows, d,
                                             _stream()),
          "rpo_reduce_groups_sets")
    return out


def attn_readonly_fwd(q, k, v, out, B: int, H: int, N: int, Kp: int, scale: float = 0.125, q_first: int = 0):
    """q_first > 0: only queries q_first .. N+Kp-1 of every image (the prompt rows when q_first = N)."""
    assert _ld(q) == _ld(k) == _ld(v)
    check(_lib.load().rpo_attn_readonly_fwd_rows(q.data_ptr(), k.data_ptr(), v.data_ptr(), _ld(q), out.data_ptr(),
                                                 _ld(out), dtype_code(q.dtype), B, H, N, Kp, scale, q_first, _stream()),
          "rpo_attn_readonly_fwd_rows")
    return out


def attn_prompt_fwd(q_rows, k, v, out, B: int, H: int, N: int, Kp: int, sets: int, first_image=None, scale: float = 0.125,
                    kv_images: Optional[int] = None):
    """The prompt queries of `sets` prompt sets (q_rows / out: [sets*B*Kp, .], set-major) over the frozen K / V of images
    first_image[0] + b (rpo_attn_prompt_fwd).  first_image: int32 device scalar or None = 0; it is read on the device, so
    the caller vouches that first_image + B <= kv_images, the images k / v hold (default: as many as their rows give)."""
    assert q_rows.dtype == k.dtype == v.dtype == out.dtype and _ld(k) == _ld(v)
    assert q_rows.shape[0] >= sets * B * Kp and out.shape[0] >= sets * B * Kp
    assert q_rows.shape[1] >= H * 64 and out.shape[1] >= H * 64 and k.shape[1] >= H * 64 and v.shape[1] >= H * 64
    kv_images = min(k.shape[0], v.shape[0]) // N if kv_images is None else kv_images
    assert B <= kv_images and min(k.shape[0], v.shape[0]) >= kv_images * N, "k / v hold fewer than B images of N rows"
    assert first_image is None or (first_image.dtype == torch.int32 and first_image.is_cuda and first_image.numel() == 1)
    check(_lib.load().rpo_attn_prompt_fwd(q_rows.data_ptr(), _ld(q_rows), k.data_ptr(), v.data_ptr(), _ld(k), out.data_ptr(),
                                          _ld(out), dtype_code(q_rows.dtype), B, H, N, Kp, sets, _p(first_image), scale,
                                          _stream()), "rpo_attn_prompt_fwd")
    return out


def attn_prompt_bwd(q_rows, k, v, da, dq, B: int, H: int, N: int, Kp: int, sets: int, first_image=None, scale: float = 0.125,
                    kv_images: Optional[int] = None):
    """The backward twin of `attn_prompt_fwd` (rpo_attn_prompt_bwd): dq of the prompt queries of `sets` prompt sets (q_rows /
    da / dq: [sets*B*Kp, .], set-major) over the frozen K / V of images first_image[0] + b; no dK / dV.  The caller vouches
    that first_image + B <= kv_images, as there."""
    assert q_rows.dtype == k.dtype == v.dtype == da.dtype == dq.dtype and _ld(k) == _ld(v)
    rows = sets * B * Kp
    assert q_rows.shape[0] >= rows and da.shape[0] >= rows and dq.shape[0] >= rows
    assert min(q_rows.shape[1], da.shape[1], dq.shape[1], k.shape[1], v.shape[1]) >= H * 64
    kv_images = min(k.shape[0], v.shape[0]) // N if kv_images is None else kv_images
    assert B <= kv_images and min(k.shape[0], v.shape[0]) >= kv_images * N, "k / v hold fewer than B images of N rows"
    assert first_image is None or (first_image.dtype == torch.int32 and first_image.is_cuda and first_image.numel() == 1)
    check(_lib.load().rpo_attn_prompt_bwd(q_rows.data_ptr(), _ld(q_rows), k.data_ptr(), v.data_ptr(), _ld(k), da.data_ptr(),
                                          _ld(da), dq.data_ptr(), _ld(dq), dtype_code(dq.dtype), B, H, N, Kp, sets,
                                          _p(first_image), scale, _stream()), "rpo_attn_prompt_bwd")
    return dq


def attn_readonly_bwd_proj(q_rows, k, v, dx, w_out_t, dq, B: int, H: int, N: int, Kp: int, scale: float = 0.125):
    """attn_readonly_bwd with the d out-proj GEMM folded in: dx = gradient of the out-proj output (act dtype)."""
    assert q_rows.dtype == k.dtype == v.dtype == dx.dtype == w_out_t.dtype == dq.dtype
    check(_lib.load().rpo_attn_readonly_bwd_proj(q_rows.data_ptr(), _ld(q_rows), k.data_ptr(), v.data_ptr(), _ld(k),
                                                 dx.data_ptr(), _ld(dx), w_out_t.data_ptr(), _ld(w_out_t), dq.data_ptr(),
                                                 _ld(dq), dtype_code(dq.dtype), B, H, N, Kp, scale, _stream()),
          "rpo_attn_readonly_bwd_proj")
    return dq


def attn_readonly_bwd(q_rows, k, v, da, dq, B: int, H: int, N: int, Kp: int, scale: float = 0.125):
    assert _ld(k) == _ld(v)
    check(_lib.load().rpo_attn_readonly_bwd(q_rows.data_ptr(), _ld(q_rows), k.data_ptr(), v.data_ptr(), _ld(k),
                                            da.data_ptr(), _ld(da), dq.data_ptr(), _ld(dq),
                                            dtype_code(q_rows.dtype), B, H, N, Kp, scale, _stream()),
          "rpo_attn_readonly_bwd")
    return dq


def chain_state() -> int:
    """bytes of device scratch rpo_chain_bwd needs (counters, placement table)"""
    return int(_lib.experimental().rpo_chain_state_bytes())


def _chain_args(layers: list, units: int, Kp: int, d: int, H: int, keys: int, dtype: torch.dtype, key_len=None,
                key_stride: int = 0, ldx: int = 0, ldq: int = 0, ldkv: int = 0, dxa=None, dxb=None, dxc=None, du=None,
                dq=None, dy=None, scale: float = 0.125, eps: float = 1e-5, wgs_per_group: int = 0, state=None,
                timeline=None):
    arr = (_lib.ChainLayer * max(1, len(layers)))()
    for i, L in enumerate(layers):
        arr[i] = _lib.ChainLayer(*[_p(L[k]) for k in ("w_proj_t", "w_fc_t", "w_out_t", "w_q_t", "aux", "x_ln2", "x_ln1",
                                                       "ln2_w", "ln1_w", "q_rows", "k", "v")])
    a = _lib.ChainBwdArgs(layer=arr, layers=len(layers), units=units, Kp=Kp, d=d, H=H, keys=keys, dtype=dtype_code(dtype),
                          key_len=_p(key_len), key_stride=key_stride, ldx=ldx, ldq=ldq, ldkv=ldkv, dxa=_p(dxa), dxb=_p(dxb),
                          dxc=_p(dxc), du=_p(du), dq=_p(dq), dy=_p(dy), dy_stride=(dy.stride(0) if dy is not None else 0),
                          scale=scale, eps=eps, wgs_per_group=wgs_per_group, state=_p(state), timeline=_p(timeline))
    a._keep = arr
    return a


def chain_bwd_ok(layers: int, units: int, Kp: int, d: int, H: int, keys: int, dtype: torch.dtype) -> bool:
    if dtype == torch.float32:
        return False
    a = _lib.ChainBwdArgs(layers=layers, units=units, Kp=Kp, d=d, H=H, keys=keys, dtype=dtype_code(dtype))
    return bool(_lib.experimental().rpo_chain_bwd_ok(C.byref(a)))


def chain_bwd(layers: list, **kw) -> None:
    """The prompt-row backward chain of one tower as one persistent launch (include/rpo_amd.h: rpo_chain_bwd).
    layers: one dict per block (block 0 first) with the tensors of struct rpo_chain_layer; x_ln2 / x_ln1 / q_rows are
    views of the back-propagated rows; dy: fp32 [4, rows, d] slabs."""
    a = _chain_args(layers, **kw)
    check(_lib.experimental().rpo_chain_bwd(C.byref(a), _stream()), "rpo_chain_bwd")


def text_attn_fwd(q, kc, vc, out, len_i32, n_cls: int, rows: int, Lmax: int, H: int, causal: bool = False,
                  scale: float = 0.125):
    assert _ld(kc) == _ld(vc) and len_i32.dtype == torch.int32
    check(_lib.load().rpo_text_attn_fwd(q.data_ptr(), _ld(q), kc.data_ptr(), vc.data_ptr(), _ld(kc),
                                        out.data_ptr(), _ld(out), dtype_code(q.dtype), len_i32.data_ptr(), n_cls,
                                        rows, Lmax, H, int(causal), scale, _stream()), "rpo_text_attn_fwd")
    return out


def text_attn_bwd_dense(q, k, v, d_out, dq, dk, dv, len_i32, n_cls: int, Lmax: int, H: int, scale: float = 0.125):
    """dq, dk, dv of the causal text attention for every row (include/rpo_amd.h: rpo_text_attn_bwd_dense)."""
    assert _ld(q) == _ld(k) == _ld(v) and _ld(dq) == _ld(dk) == _ld(dv) and len_i32.dtype == torch.int32
    assert q.dtype == d_out.dtype == dq.dtype
    check(_lib.load().rpo_text_attn_bwd_dense(q.data_ptr(), k.data_ptr(), v.data_ptr(), _ld(q), d_out.data_ptr(),
                                              _ld(d_out), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), _ld(dq),
                                              dtype_code(q.dtype), len_i32.data_ptr(), n_cls, Lmax, H, scale, _stream()),
          "rpo_text_attn_bwd_dense")
    return dq


def text_attn_bwd(q, kc, vc, da, dq, len_i32, n_cls: int, rows: int, Lmax: int, H: int, scale: float = 0.125):
    assert _ld(kc) == _ld(vc) and len_i32.dtype == torch.int32
    check(_lib.load().rpo_text_attn_bwd(q.data_ptr(), _ld(q), kc.data_ptr(), vc.data_ptr(), _ld(kc),
                                        da.data_ptr(), _ld(da), dq.data_ptr(), _ld(dq), dtype_code(q.dtype),
                                        len_i32.data_ptr(), n_cls, rows, Lmax, H, scale, _stream()),
          "rpo_text_attn_bwd")
    return dq


def text_attn_fwd_shared(q, kc, vc, out, len_i32, n_cls: int, n_kv: int, rows: int, Lmax: int, H: int, scale: float = 0.125):
    """`text_attn_fwd` (causal = False) for n_cls virtual classes on the cache of n_kv real ones (rpo_text_attn_fwd_shared)."""
    assert _ld(kc) == _ld(vc) and len_i32.dtype == torch.int32 and len_i32.numel() >= n_kv
    assert kc.shape[0] >= n_kv * Lmax and q.shape[0] >= n_cls * rows and out.shape[0] >= n_cls * rows
    check(_lib.load().rpo_text_attn_fwd_shared(q.data_ptr(), _ld(q), kc.data_ptr(), vc.data_ptr(), _ld(kc),
                                               out.data_ptr(), _ld(out), dtype_code(q.dtype), len_i32.data_ptr(), n_cls,
                                               n_kv, rows, Lmax, H, scale, _stream()), "rpo_text_attn_fwd_shared")
    return out


def text_attn_fwd_prefix(q, k, v, out, len_i32, n_img: int, n_cls: int, P: int, S: int, H: int, scale: float = 0.125):
    """The causal text attention of n_img * n_cls sequences whose first P rows are shared by the classes of an image
    (include/rpo_amd.h: rpo_text_attn_fwd_prefix): n_img * P prefix rows, then n_img * n_cls * S suffix rows."""
    rows = n_img * P + n_img * n_cls * S
    assert _ld(q) == _ld(k) == _ld(v) and len_i32.dtype == torch.int32 and len_i32.numel() >= n_cls
    assert q.dtype == k.dtype == v.dtype == out.dtype
    assert min(q.shape[0], k.shape[0], v.shape[0], out.shape[0]) >= rows and min(q.shape[1], out.shape[1]) >= H * 64
    check(_lib.load().rpo_text_attn_fwd_prefix(q.data_ptr(), k.data_ptr(), v.data_ptr(), _ld(q), out.data_ptr(), _ld(out),
                                               dtype_code(q.dtype), len_i32.data_ptr(), n_img, n_cls, P, S, H, scale,
                                               _stream()), "rpo_text_attn_fwd_prefix")
    return out


def text_attn_bwd_prefix_workspace_floats(n_img: int, n_cls: int, P: int, H: int) -> int:
    return int(_lib.load().rpo_text_attn_bwd_prefix_workspace_floats(n_img, n_cls, P, H))


def text_attn_bwd_prefix(q, k, v, d_out, dq, dk, dv, len_i32, n_img: int, n_cls: int, P: int, S: int, H: int,
                         scale: float = 0.125, workspace=None):
    """dq, dk, dv of `text_attn_fwd_prefix`'s attention on its row layout, the prefix rows' dk / dv summed over the classes
    (include/rpo_amd.h: rpo_text_attn_bwd_prefix).  `workspace`: fp32, text_attn_bwd_prefix_workspace_floats(...) elements
    (allocated here when not given)."""
    rows = n_img * P + n_img * n_cls * S
    assert _ld(q) == _ld(k) == _ld(v) and _ld(dq) == _ld(dk) == _ld(dv) and len_i32.dtype == torch.int32
    assert len_i32.numel() >= n_cls and q.dtype == k.dtype == v.dtype == d_out.dtype == dq.dtype == dk.dtype == dv.dtype
    assert min(t.shape[0] for t in (q, k, v, d_out, dq, dk, dv)) >= rows
    assert min(t.shape[1] for t in (q, k, v, d_out, dq, dk, dv)) >= H * 64
    need = text_attn_bwd_prefix_workspace_floats(n_img, n_cls, P, H)
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.float32, device=q.device)
    assert workspace.dtype == torch.float32 and workspace.is_contiguous() and workspace.numel() >= need
    check(_lib.load().rpo_text_attn_bwd_prefix(q.data_ptr(), k.data_ptr(), v.data_ptr(), _ld(q), d_out.data_ptr(),
                                               _ld(d_out), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), _ld(dq),
                                               dtype_code(q.dtype), len_i32.data_ptr(), n_img, n_cls, P, S, H, scale,
                                               workspace.data_ptr(), _stream()), "rpo_text_attn_bwd_prefix")
    return dq


def text_attn_bwd_shared(q, kc, vc, da, dq, len_i32, n_cls: int, n_kv: int, rows: int, Lmax: int, H: int, scale: float = 0.125):
    """`text_attn_bwd` for n_cls virtual classes on the cache of n_kv real ones (rpo_text_attn_bwd_shared)."""
    assert _ld(kc) == _ld(vc) and len_i32.dtype == torch.int32 and len_i32.numel() >= n_kv
    assert kc.shape[0] >= n_kv * Lmax and q.shape[0] >= n_cls * rows and da.shape[0] >= n_cls * rows and dq.shape[0] >= n_cls * rows
    check(_lib.load().rpo_text_attn_bwd_shared(q.data_ptr(), _ld(q), kc.data_ptr(), vc.data_ptr(), _ld(kc),
                                               da.data_ptr(), _ld(da), dq.data_ptr(), _ld(dq), dtype_code(q.dtype),
                                               len_i32.data_ptr(), n_cls, n_kv, rows, Lmax, H, scale, _stream()),
          "rpo_text_attn_bwd_shared")
    return dq


def head_workspace_floats(B: int, Cc: int, K: int, e: int) -> int:
    return int(_lib.load().rpo_head_workspace_floats(B, Cc, K, e))


def head_fwd_bwd(img_f, text_f, label, scale_exp: float, logits, loss, d_img_f, d_text_f, ws,
                 d_img_f_act=None, d_text_f_act=None):
    """d_*_act: optional act-dtype copies of the two gradients (what the projections' dX GEMMs read)."""
    B, K, e = img_f.shape
    Cc = text_f.shape[0]
    assert img_f.is_contiguous() and text_f.is_contiguous() and logits.is_contiguous()
    assert label is None or label.dtype == torch.int64
    act = d_img_f_act if d_img_f_act is not None else d_text_f_act
    assert act is None or (act.is_contiguous() and (d_text_f_act is None or d_text_f_act.is_contiguous()))
    check(_lib.load().rpo_head_fwd_bwd_act(img_f.data_ptr(), text_f.data_ptr(), _p(label), scale_exp,
                                           logits.data_ptr(), _p(loss), _p(d_img_f), _p(d_text_f), _p(d_img_f_act),
                                           _p(d_text_f_act), _lib.RPO_F32 if act is None else dtype_code(act.dtype),
                                           B, Cc, K, e, ws.data_ptr(), _stream()), "rpo_head_fwd_bwd_act")
    return logits


def head_fwd_bwd_grouped(img_f, text_f, label, scale_exp: float, logits, loss, d_img_f, d_text_f, ws, S: int,
                         d_img_f_act=None, d_text_f_act=None, k_used=None):
    """S independent heads in one call (rpo_head_fwd_bwd_grouped[_act]): img_f [S*B, K, e], text_f [S*C, K, e], label [S*B]
    or None, logits [S*B, C], loss [S]; ws: S * head_workspace_floats(B, C, K, e) floats.  k_used: int32 [S] on the device
    -- group s pairs only its first k_used[s] of the K rows (rpo_head_fwd_bwd_grouped_k); None: the entry point without."""
    SB, K, e = img_f.shape
    assert SB % S == 0 and text_f.shape[0] % S == 0
    B, Cc = SB // S, text_f.shape[0] // S
    assert img_f.is_contiguous() and text_f.is_contiguous() and logits.is_contiguous() and logits.numel() >= SB * Cc
    assert label is None or (label.dtype == torch.int64 and label.numel() == SB and label.is_contiguous())
    assert label is None or (loss.numel() >= S and loss.is_contiguous())
    assert ws.numel() >= S * head_workspace_floats(B, Cc, K, e)
    act = d_img_f_act if d_img_f_act is not None else d_text_f_act
    assert act is None or (act.is_contiguous() and (d_text_f_act is None or d_text_f_act.is_contiguous()))
    if k_used is not None:
        assert k_used.dtype == torch.int32 and k_used.is_cuda and k_used.numel() == S and k_used.is_contiguous()
        check(_lib.load().rpo_head_fwd_bwd_grouped_k(img_f.data_ptr(), text_f.data_ptr(), _p(label), scale_exp,
                                                     logits.data_ptr(), _p(loss), _p(d_img_f), _p(d_text_f),
                                                     _p(d_img_f_act), _p(d_text_f_act),
                                                     _lib.RPO_F32 if act is None else dtype_code(act.dtype),
                                                     S, B, Cc, K, e, k_used.data_ptr(), ws.data_ptr(), _stream()),
              "rpo_head_fwd_bwd_grouped_k")
        return logits
    check(_lib.load().rpo_head_fwd_bwd_grouped_act(img_f.data_ptr(), text_f.data_ptr(), _p(label), scale_exp,
                                                   logits.data_ptr(), _p(loss), _p(d_img_f), _p(d_text_f),
                                                   _p(d_img_f_act), _p(d_text_f_act),
                                                   _lib.RPO_F32 if act is None else dtype_code(act.dtype),
                                                   S, B, Cc, K, e, ws.data_ptr(), _stream()), "rpo_head_fwd_bwd_grouped_act")
    return logits


def lp_head_workspace_floats(B: int, Cc: int, e: int) -> int:
    return int(_lib.load().rpo_lp_head_workspace_floats(B, Cc, e))


def lp_head_fwd_bwd(img_f, w, bias, text_f_n, label, scale_exp: float, z, logits, loss, g_w, g_bias, ws):
    """The linear-probe head (include/rpo_amd.h rpo_lp_head_fwd_bwd): label None = eval (z and logits only)."""
    B, e = img_f.shape
    Cc = text_f_n.shape[0]
    assert w.shape == (e, e) and bias.shape == (e,) and text_f_n.shape == (Cc, e)
    assert z.shape == (B, e) and logits.shape == (B, Cc)
    ts = [img_f, w, bias, text_f_n, z, logits] + ([] if label is None else [loss, g_w, g_bias])
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in ts + [ws])
    assert label is None or (label.dtype == torch.int64 and label.numel() == B)
    assert label is None or (g_w.shape == (e, e) and g_bias.shape == (e,))
    assert ws.numel() >= lp_head_workspace_floats(B, Cc, e)
    check(_lib.load().rpo_lp_head_fwd_bwd(img_f.data_ptr(), w.data_ptr(), bias.data_ptr(), text_f_n.data_ptr(), _p(label),
                                          scale_exp, z.data_ptr(), logits.data_ptr(), _p(loss), _p(g_w), _p(g_bias),
                                          B, Cc, e, ws.data_ptr(), _stream()), "rpo_lp_head_fwd_bwd")
    return logits


def lp_head_fwd_bwd_grouped(img_f, params, text_f_n, label, scale_exp: float, z, logits, loss, grads, ws):
    """S linear-probe heads in the launches of one (include/rpo_amd.h rpo_lp_head_fwd_bwd_grouped): params / grads
    [S, stride >= e e + e] fp32 with one row stride, row s = [W_s | b_s]; z [S, B, e], logits [S, B, C], loss [S]; img_f,
    text_f_n and label are shared.  label None = eval (z and logits only)."""
    B, e = img_f.shape
    Cc = text_f_n.shape[0]
    S, stride = params.shape[0], params.stride(0)
    assert params.dim() == 2 and params.stride(1) == 1 and params.shape[1] >= e * e + e and text_f_n.shape == (Cc, e)
    assert z.shape == (S, B, e) and logits.shape == (S, B, Cc)
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in [img_f, text_f_n, z, logits, ws])
    assert params.dtype == torch.float32
    if label is not None:
        assert label.dtype == torch.int64 and label.numel() == B and loss.dtype == torch.float32 and loss.numel() == S
        assert loss.is_contiguous() and grads.dtype == torch.float32 and grads.shape[0] == S and grads.stride(1) == 1
        assert grads.stride(0) == stride and grads.shape[1] >= e * e + e, "grads has the layout of params"
    assert ws.numel() >= S * lp_head_workspace_floats(B, Cc, e)
    check(_lib.load().rpo_lp_head_fwd_bwd_grouped(img_f.data_ptr(), params.data_ptr(), stride, text_f_n.data_ptr(),
                                                  _p(label), scale_exp, z.data_ptr(), logits.data_ptr(), _p(loss),
                                                  _p(grads), S, B, Cc, e, ws.data_ptr(), _stream()),
          "rpo_lp_head_fwd_bwd_grouped")
    return logits


def text_ensemble_accumulate(feat, n_cls: int, acc, first: bool = True, template_stride_rows: Optional[int] = None):
    """Prompt ensembling, first half (include/rpo_amd.h rpo_text_ensemble_accumulate): feat [rows, e] fp32 (row stride >= e)
    holds T blocks of n_cls rows, block t at row t * template_stride_rows (default n_cls: T = rows / n_cls); adds every
    block's L2-normalised rows to acc [n_cls, e] in ascending t (first: acc starts from zero).  Enqueue only."""
    stride = n_cls if template_stride_rows is None else int(template_stride_rows)
    assert feat.dim() == 2 and feat.dtype == torch.float32 and feat.stride(1) == 1 and n_cls >= 1 and stride >= n_cls
    e = feat.shape[1]
    T = (feat.shape[0] - n_cls) // stride + 1
    assert T >= 1 and (T - 1) * stride + n_cls <= feat.shape[0], "feat holds no whole block of n_cls rows"
    assert acc.dtype == torch.float32 and acc.shape == (n_cls, e) and acc.is_contiguous() and acc.device == feat.device
    check(_lib.load().rpo_text_ensemble_accumulate(feat.data_ptr(), feat.stride(0), T, stride, n_cls, e, acc.data_ptr(),
                                                   1 if first else 0, _stream()), "rpo_text_ensemble_accumulate")
    return acc


def text_ensemble_finish(acc, T_total: int, out=None):
    """Prompt ensembling, second half (rpo_text_ensemble_finish): out = normalise(acc / T_total); out None: in place."""
    out = acc if out is None else out
    n_cls, e = acc.shape
    assert acc.dtype == torch.float32 and acc.is_contiguous()
    assert out.dtype == torch.float32 and out.shape == acc.shape and out.is_contiguous() and out.device == acc.device
    check(_lib.load().rpo_text_ensemble_finish(acc.data_ptr(), n_cls, e, int(T_total), out.data_ptr(), _stream()),
          "rpo_text_ensemble_finish")
    return out


def eval_accumulate(logits, label, counts, cmat=None, pred=None):
    """The classification evaluator's device half (include/rpo_amd.h rpo_eval_accumulate): counts int64 [2] (correct, total)
    and cmat int32 [C, C] (row = true class) accumulate; pred int32 [B] is overwritten.  Enqueue only."""
    B, Cc = logits.shape
    assert logits.dtype == torch.float32 and logits.stride(1) == 1
    assert label.dtype == torch.int64 and label.numel() == B and label.is_contiguous()
    assert counts.dtype == torch.int64 and counts.numel() == 2 and counts.is_contiguous()
    assert cmat is None or (cmat.dtype == torch.int32 and cmat.numel() == Cc * Cc and cmat.is_contiguous())
    assert pred is None or (pred.dtype == torch.int32 and pred.numel() == B and pred.is_contiguous())
    check(_lib.load().rpo_eval_accumulate(logits.data_ptr(), logits.stride(0), label.data_ptr(), B, Cc, counts.data_ptr(),
                                          _p(cmat), _p(pred), _stream()), "rpo_eval_accumulate")
    return counts


def features_classify(feat, cls, bias, label, scale: float, norm_feat: bool, norm_cls: bool, counts, cmat=None, pred=None,
                      logits_out=None):
    """S classifiers over cached image features, head and evaluator in one launch (include/rpo_amd.h
    rpo_features_classify): feat [n, e] fp32 (row stride >= e), cls [S, C, e], bias [S, C] or None, label int64 [n];
    counts int64 [S, 2] and cmat int32 [S, C, C] accumulate, pred int32 [S, n] and logits_out [S, n, C] are overwritten.
    Enqueue only."""
    n, e = feat.shape
    S, Cc = cls.shape[0], cls.shape[1]
    assert feat.dtype == torch.float32 and feat.stride(1) == 1
    assert cls.dtype == torch.float32 and cls.shape == (S, Cc, e) and cls.is_contiguous() and cls.device == feat.device
    assert bias is None or (bias.dtype == torch.float32 and bias.shape == (S, Cc) and bias.is_contiguous())
    assert label.dtype == torch.int64 and label.numel() == n and label.is_contiguous()
    assert counts.dtype == torch.int64 and counts.numel() == 2 * S and counts.is_contiguous()
    assert cmat is None or (cmat.dtype == torch.int32 and cmat.numel() == S * Cc * Cc and cmat.is_contiguous())
    assert pred is None or (pred.dtype == torch.int32 and pred.numel() == S * n and pred.is_contiguous())
    assert logits_out is None or (logits_out.dtype == torch.float32 and logits_out.numel() == S * n * Cc
                                  and logits_out.is_contiguous())
    check(_lib.load().rpo_features_classify(feat.data_ptr(), feat.stride(0), cls.data_ptr(), _p(bias), label.data_ptr(),
                                            float(scale), int(bool(norm_feat)), int(bool(norm_cls)), counts.data_ptr(),
                                            _p(cmat), _p(pred), _p(logits_out), n, Cc, e, S, _stream()),
          "rpo_features_classify")
    return counts


def logreg_workspace_floats(n: int, Cc: int, e: int, S: int) -> int:
    return int(_lib.load().rpo_logreg_workspace_floats(n, Cc, e, S))


def logreg_loss_grad_sets(feat, label, weight, omega, l2, params, n_cls: int, grads, loss, ws, norm_feat: bool = False,
                          fit_bias: bool = True, done=None):
    """Loss and gradient of S multinomial logistic regressions on cached features (include/rpo_amd.h
    rpo_logreg_loss_grad_sets): feat [n, e] fp32 (row stride >= e), label int64 [n], weight [S, n] fp32 or None, omega
    float64 [S], l2 fp32 [S], params / grads [S, stride] fp32 with row s = [W_s (n_cls x e) | b_s (n_cls)], loss fp32 [S],
    done int32 [S] or None.  Enqueue only."""
    n, e = feat.shape
    S = params.shape[0]
    assert feat.dtype == torch.float32 and feat.stride(1) == 1
    assert label.dtype == torch.int64 and label.numel() == n and label.is_contiguous()
    assert weight is None or (weight.dtype == torch.float32 and weight.shape == (S, n) and weight.is_contiguous())
    assert omega.dtype == torch.float64 and omega.numel() == S and omega.is_contiguous()
    assert l2.dtype == torch.float32 and l2.numel() == S and l2.is_contiguous()
    assert params.dtype == torch.float32 and params.dim() == 2 and params.stride(1) == 1
    assert grads.dtype == torch.float32 and grads.shape == params.shape and grads.stride() == params.stride()
    assert loss.dtype == torch.float32 and loss.numel() == S and loss.is_contiguous()
    assert done is None or (done.dtype == torch.int32 and done.numel() == S and done.is_contiguous())
    assert ws.dtype == torch.float32 and ws.is_contiguous() and ws.numel() >= logreg_workspace_floats(n, n_cls, e, S)
    check(_lib.load().rpo_logreg_loss_grad_sets(feat.data_ptr(), feat.stride(0), label.data_ptr(), _p(weight),
                                                omega.data_ptr(), l2.data_ptr(), params.data_ptr(), params.stride(0),
                                                _p(done), int(bool(norm_feat)), int(bool(fit_bias)), grads.data_ptr(),
                                                loss.data_ptr(), n, int(n_cls), e, S, ws.data_ptr(), _stream()),
          "rpo_logreg_loss_grad_sets")
    return loss


def logreg_step_sets(x, y, grads, count: int, t, L, tol, done, iters, grad_inf):
    """One accelerated-gradient iteration with gradient restart per member (include/rpo_amd.h rpo_logreg_step_sets) on
    rows x, y, grads [S, stride] fp32 (`count` valid floats each); t, L, tol, grad_inf fp32 [S], done, iters int32 [S].
    Enqueue only."""
    S = x.shape[0]
    for a in (x, y, grads):
        assert a.dtype == torch.float32 and a.dim() == 2 and a.shape[0] == S and a.stride() == x.stride() and a.stride(1) == 1
    for a in (t, L, tol, grad_inf):
        assert a.dtype == torch.float32 and a.numel() == S and a.is_contiguous()
    for a in (done, iters):
        assert a.dtype == torch.int32 and a.numel() == S and a.is_contiguous()
    check(_lib.load().rpo_logreg_step_sets(x.data_ptr(), y.data_ptr(), grads.data_ptr(), x.stride(0), int(count),
                                           t.data_ptr(), L.data_ptr(), tol.data_ptr(), done.data_ptr(), iters.data_ptr(),
                                           grad_inf.data_ptr(), S, _stream()),
          "rpo_logreg_step_sets")


def metanet_fwd(img_f, w1, b1, w2, b2, f_norm, hidden, bias):
    B, e = img_f.shape
    h, d = w1.shape[0], w2.shape[0]
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (img_f, w1, b1, w2, b2, f_norm, hidden, bias))
    check(_lib.load().rpo_metanet_fwd(img_f.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                                      f_norm.data_ptr(), hidden.data_ptr(), bias.data_ptr(), B, e, h, d, _stream()),
          "rpo_metanet_fwd")
    return bias


def metanet_bwd(d_bias, f_norm, hidden, w2, g_w1, g_b1, g_w2, g_b2):
    B, d = d_bias.shape
    e, h = f_norm.shape[1], hidden.shape[1]
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (d_bias, f_norm, hidden, w2, g_w1, g_b1, g_w2, g_b2))
    check(_lib.load().rpo_metanet_bwd(d_bias.data_ptr(), f_norm.data_ptr(), hidden.data_ptr(), w2.data_ptr(),
                                      g_w1.data_ptr(), g_b1.data_ptr(), g_w2.data_ptr(), g_b2.data_ptr(), B, e, h, d,
                                      _stream()), "rpo_metanet_bwd")


def _sets_rows(params, what: str = "params"):
    """(S, row stride) of a members' buffer [S, stride] whose rows the *_sets entry points address by one stride."""
    assert params.dim() == 2 and params.dtype == torch.float32 and params.stride(1) == 1, f"{what} is fp32 [S, set_stride]"
    return params.shape[0], params.stride(0)


def metanet_fwd_sets(img_f, params, n_ctx: int, f_norm, hidden, bias, b: int):
    """The meta-net of S members on b images each (include/rpo_amd.h rpo_metanet_fwd_sets): img_f [S*b, e] member-major,
    params [S, set_stride] with row s = [ctx | w1 | b1 | w2 | b2]; writes f_norm [S*b, e], hidden [S*b, h], bias [S*b, d]."""
    S, stride = _sets_rows(params)
    SB, e = img_f.shape
    h, d = hidden.shape[1], bias.shape[1]
    assert SB == S * b and f_norm.shape == (SB, e) and hidden.shape == (SB, h) and bias.shape == (SB, d)
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (img_f, f_norm, hidden, bias))
    check(_lib.load().rpo_metanet_fwd_sets(img_f.data_ptr(), params.data_ptr(), stride, n_ctx, f_norm.data_ptr(),
                                           hidden.data_ptr(), bias.data_ptr(), S, b, e, h, d, _stream()),
          "rpo_metanet_fwd_sets")
    return bias


def cocoop_shift_sets(params, bias, c_shift, b: int):
    """c_shift[s b + i, r, :] = ctx_s[r, :] + bias[s b + i, :] in one launch (rpo_cocoop_shift_sets): params [S, set_stride],
    bias [S*b, d], c_shift [S*b, n_ctx, d]."""
    S, stride = _sets_rows(params)
    SB, n_ctx, d = c_shift.shape
    assert SB == S * b and bias.shape == (SB, d)
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (bias, c_shift))
    check(_lib.load().rpo_cocoop_shift_sets(params.data_ptr(), stride, bias.data_ptr(), c_shift.data_ptr(), S, b, n_ctx, d,
                                            _stream()), "rpo_cocoop_shift_sets")
    return c_shift


def cocoop_grad_tail_sets(d_shift, loss_img, grads, d_bias, loss, b: int):
    """The members' gradient tail in one launch (rpo_cocoop_grad_tail_sets): d_shift [S*b, n_ctx, d], loss_img [S*b] ->
    the ctx part of row s of grads [S, set_stride], d_bias [S*b, d], loss [S] (means over the member's b images)."""
    S, stride = _sets_rows(grads, "grads")
    SB, n_ctx, d = d_shift.shape
    assert SB == S * b and loss_img.numel() == SB and d_bias.shape == (SB, d) and loss.numel() == S
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (d_shift, loss_img, d_bias, loss))
    check(_lib.load().rpo_cocoop_grad_tail_sets(d_shift.data_ptr(), loss_img.data_ptr(), grads.data_ptr(), stride,
                                                d_bias.data_ptr(), loss.data_ptr(), S, b, n_ctx, d, _stream()),
          "rpo_cocoop_grad_tail_sets")


def metanet_bwd_sets(d_bias, f_norm, hidden, params, grads, n_ctx: int, b: int):
    """The meta-net backward of S members (rpo_metanet_bwd_sets): per member rpo_metanet_bwd(B = b) on its slices, written
    into row s of grads [S, set_stride] (the layout and stride of params)."""
    S, stride = _sets_rows(params)
    SB, d = d_bias.shape
    e, h = f_norm.shape[1], hidden.shape[1]
    assert SB == S * b and f_norm.shape == (SB, e) and hidden.shape == (SB, h)
    assert _sets_rows(grads, "grads") == (S, stride), "grads has the layout of params"
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (d_bias, f_norm, hidden))
    check(_lib.load().rpo_metanet_bwd_sets(d_bias.data_ptr(), f_norm.data_ptr(), hidden.data_ptr(), params.data_ptr(),
                                           grads.data_ptr(), stride, n_ctx, S, b, e, h, d, _stream()),
          "rpo_metanet_bwd_sets")


def coop_fill_sets(tok, pos, params, n_ctx_members, x0, n_cls: int, L: int, n_max: int):
    """The input rows of a dense text pass over S CoOp members with their own n_ctx (include/rpo_amd.h rpo_coop_fill_sets):
    tok [n_cls * L, d], pos [L, d], params [S, set_stride], n_ctx_members int32 [S] on the device -> x0 [S * n_cls * L, d]."""
    S, stride = _sets_rows(params)
    d = tok.shape[1]
    assert tok.shape == (n_cls * L, d) and pos.shape == (L, d) and x0.shape == (S * n_cls * L, d)
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (tok, pos, x0))
    assert n_ctx_members.dtype == torch.int32 and n_ctx_members.is_cuda and n_ctx_members.numel() == S \
        and n_ctx_members.is_contiguous()
    check(_lib.load().rpo_coop_fill_sets(tok.data_ptr(), pos.data_ptr(), params.data_ptr(), stride, n_ctx_members.data_ptr(),
                                         x0.data_ptr(), S, n_cls, L, n_max, d, _stream()), "rpo_coop_fill_sets")
    return x0


def coop_ctx_grad_sets(dx, grads, n_ctx_members, n_cls: int, L: int, n_max: int):
    """The members' context gradients in one launch (rpo_coop_ctx_grad_sets): dx [S * n_cls * L, d] read in place -> the first
    n_max * d floats of row s of grads [S, set_stride], in rpo_reduce_groups's summation order, the unused tail zeroed."""
    S, stride = _sets_rows(grads, "grads")
    d = dx.shape[1]
    assert dx.shape == (S * n_cls * L, d) and dx.dtype == torch.float32 and dx.is_contiguous()
    assert n_ctx_members.dtype == torch.int32 and n_ctx_members.is_cuda and n_ctx_members.numel() == S \
        and n_ctx_members.is_contiguous()
    check(_lib.load().rpo_coop_ctx_grad_sets(dx.data_ptr(), grads.data_ptr(), stride, n_ctx_members.data_ptr(), S, n_cls, L,
                                             n_max, d, _stream()), "rpo_coop_ctx_grad_sets")
    return grads


def sgd_step(p, g, buf, lr: float, momentum: float, wd: float, grad_scale: float, first_step: bool):
    assert p.is_contiguous() and g.is_contiguous() and buf.is_contiguous()
    check(_lib.load().rpo_sgd_step(p.data_ptr(), g.data_ptr(), buf.data_ptr(), p.numel(), lr, momentum, wd,
                                   grad_scale, int(first_step), _stream()), "rpo_sgd_step")
    return p


def sgd_step_guarded(p, g, buf, lr: float, momentum: float, wd: float, grad_scale: float, first_step: bool, found_inf):
    """sgd_step, skipped as a whole when a gradient is Inf / NaN (GradScaler.step); found_inf: int32[2] device tensor."""
    assert p.is_contiguous() and g.is_contiguous() and buf.is_contiguous()
    assert found_inf.dtype == torch.int32 and found_inf.numel() >= 2 and found_inf.is_contiguous()
    check(_lib.load().rpo_sgd_step_guarded(p.data_ptr(), g.data_ptr(), buf.data_ptr(), p.numel(), lr, momentum, wd,
                                           grad_scale, int(first_step), found_inf.data_ptr(), _stream()),
          "rpo_sgd_step_guarded")
    return p


def sgd_step_sets(p, g, buf, hyper, seg0: int, seg1: int, first_step: bool, used=None, found_inf=None):
    """rpo_sgd_step_sets: p / g / buf [sets, >= seg0 + seg1] fp32 with one row stride; hyper float32 [sets, 4] (lr, momentum,
    weight decay, grad_scale), used int32 [sets, 2] or None, found_inf int32 [sets, 2] or None -- all on the device."""
    sets, stride = p.shape[0], p.stride(0)
    for t in (p, g, buf):
        assert t.dtype == torch.float32 and t.dim() == 2 and t.shape[0] == sets and t.stride() == (stride, 1)
        assert t.shape[1] >= seg0 + seg1
    assert hyper.dtype == torch.float32 and hyper.is_cuda and tuple(hyper.shape) == (sets, 4) and hyper.is_contiguous()
    for t in (used, found_inf):
        assert t is None or (t.dtype == torch.int32 and t.is_cuda and tuple(t.shape) == (sets, 2) and t.is_contiguous())
    check(_lib.load().rpo_sgd_step_sets(p.data_ptr(), g.data_ptr(), buf.data_ptr(), stride, sets, hyper.data_ptr(), _p(used),
                                        seg0, seg1, int(first_step), _p(found_inf), _stream()), "rpo_sgd_step_sets")
    return p


def optim_step_sets(p, g, s0, s1, s2, kind, hyper, step, seg0: int, seg1: int, used=None, found_inf=None,
                    needs_s2: bool = False):
    """rpo_optim_step_sets: p / g / s0 / s1 (/ s2 or None) [sets, >= seg0 + seg1] fp32 with one row stride; kind int32 [sets],
    hyper float32 [sets, 8], step int32 [sets], used / found_inf int32 [sets, 2] or None -- all on the device (columns and
    rules: include/rpo_amd.h)."""
    sets, stride = p.shape[0], p.stride(0)
    for t in (p, g, s0, s1) + (() if s2 is None else (s2,)):
        assert t.dtype == torch.float32 and t.dim() == 2 and t.shape[0] == sets and t.stride() == (stride, 1)
        assert t.shape[1] >= seg0 + seg1
    assert hyper.dtype == torch.float32 and hyper.is_cuda and tuple(hyper.shape) == (sets, 8) and hyper.is_contiguous()
    for t in (kind, step):
        assert t.dtype == torch.int32 and t.is_cuda and tuple(t.shape) == (sets,) and t.is_contiguous()
    for t in (used, found_inf):
        assert t is None or (t.dtype == torch.int32 and t.is_cuda and tuple(t.shape) == (sets, 2) and t.is_contiguous())
    check(_lib.load().rpo_optim_step_sets(p.data_ptr(), g.data_ptr(), s0.data_ptr(), s1.data_ptr(), _p(s2), stride, sets,
                                          kind.data_ptr(), hyper.data_ptr(), step.data_ptr(), _p(used), seg0, seg1,
                                          int(needs_s2), _p(found_inf), _stream()), "rpo_optim_step_sets")
    return p


def convert(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    assert src.dtype == torch.float32 and src.shape == dst.shape
    check(_lib.load().rpo_convert(src.data_ptr(), _ld(src), dst.data_ptr(), dtype_code(dst.dtype), _ld(dst),
                                  src.shape[0], src.shape[1], _stream()), "rpo_convert")
    return dst


def probe_mfma(which: int, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    d = torch.empty(32, 32, dtype=torch.float32, device=a.device)
    check(_lib.load().rpo_probe_mfma(which, a.data_ptr(), b.data_ptr(), d.data_ptr(), _stream()),
          "rpo_probe_mfma")
    return d


def probe_peaks(device: torch.device, which: int = 0, copy: bool = True) -> dict:
    """Empirical peaks of this GPU: sustained MFMA TFLOP/s of a pure-MFMA loop (8 waves per SIMD-pair resident,
    non-zero operands) and GB/s of a 1 GiB stream copy (read + write bytes).  ~0.2 s."""
    import ctypes
    lib = _lib.load()
    sink = torch.zeros(4, dtype=torch.float32, device=device)
    flops = ctypes.c_double(0.0)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    blocks, iters = 256 * 8, 4096 if which != 1 else 2048
    for timed in (False, True):
        if timed:
            ev[0].record()
        check(lib.rpo_probe_peak_mfma(which, blocks, iters, sink.data_ptr(), ctypes.byref(flops), _stream()),
              "rpo_probe_peak_mfma")
        if timed:
            ev[1].record()
    if not copy:
        torch.cuda.synchronize(device)
        return {"mfma_tflops": flops.value / (ev[0].elapsed_time(ev[1]) * 1e-3) / 1e12}
    n = 1 << 29
    src = torch.empty(n, dtype=torch.uint8, device=device).fill_(1)
    dst = torch.empty_like(src)
    reps = 5
    for timed in (False, True):
        if timed:
            ev[2].record()
        for _ in range(reps if timed else 1):
            check(lib.rpo_probe_peak_copy(src.data_ptr(), dst.data_ptr(), n, _stream()), "rpo_probe_peak_copy")
        if timed:
            ev[3].record()
    torch.cuda.synchronize(device)
    return {"mfma_tflops": flops.value / (ev[0].elapsed_time(ev[1]) * 1e-3) / 1e12,
            "copy_gbs": 2.0 * n * reps / (ev[2].elapsed_time(ev[3]) * 1e-3) / 1e9}


# ---- CLIP ResNet image tower (include/rpo_amd.h, csrc/conv.hip) --------------------------------------------------------

def _nhwc(t: torch.Tensor, what: str) -> None:
    assert t.is_cuda and t.is_contiguous() and t.dim() == 4, f"{what}: contiguous [B, H, W, C] device tensor"


def conv2d_nhwc(x, w, bias, y, resid=None, relu: bool = True, tile_config: int = 0):
    """y = relu?(conv(x, w) + bias [+ resid]) (include/rpo_amd.h rpo_conv2d_nhwc): x [B,H,W,Cin], w [Cout,k,k,Cin] act dtype,
    bias fp32 [Cout], resid / y [B,H,W,Cout]."""
    _nhwc(x, "x"); _nhwc(y, "y")
    B, H, W, Cin = x.shape
    Cout, kh, kw, cin_w = w.shape
    assert kh == kw and cin_w == Cin and w.is_contiguous() and w.dtype == x.dtype == y.dtype
    assert tuple(y.shape) == (B, H, W, Cout) and bias.dtype == torch.float32 and bias.numel() == Cout
    if resid is not None:
        _nhwc(resid, "resid")
        assert resid.shape == y.shape and resid.dtype == y.dtype
    check(_lib.load().rpo_conv2d_nhwc(x.data_ptr(), w.data_ptr(), bias.data_ptr(), _p(resid), y.data_ptr(),
                                      dtype_code(x.dtype), B, H, W, Cin, Cout, kh, int(relu), tile_config, _stream()),
          "rpo_conv2d_nhwc")
    return y


def conv_stem(image, w, bias, y, relu: bool = True):
    """Stem conv1 (rpo_conv_stem): fp32 NCHW image [B,3,H,W] -> y [B,H/2,W/2,Cout] NHWC, w [Cout,3,3,3] act dtype."""
    assert image.dtype == torch.float32 and image.is_contiguous() and image.dim() == 4 and image.shape[1] == 3
    _nhwc(y, "y")
    B, _, H, W = image.shape
    Cout = w.shape[0]
    assert tuple(w.shape) == (Cout, 3, 3, 3) and w.is_contiguous() and w.dtype == y.dtype
    assert tuple(y.shape) == (B, H // 2, W // 2, Cout) and bias.dtype == torch.float32 and bias.numel() == Cout
    check(_lib.load().rpo_conv_stem(image.data_ptr(), w.data_ptr(), bias.data_ptr(), y.data_ptr(), dtype_code(y.dtype),
                                    B, H, W, Cout, int(relu), _stream()), "rpo_conv_stem")
    return y


def avgpool_nhwc(x, y, k: int):
    """AvgPool2d(k) on NHWC (rpo_avgpool_nhwc)."""
    _nhwc(x, "x"); _nhwc(y, "y")
    B, H, W, C = x.shape
    assert tuple(y.shape) == (B, H // k, W // k, C) and y.dtype == x.dtype
    check(_lib.load().rpo_avgpool_nhwc(x.data_ptr(), y.data_ptr(), dtype_code(x.dtype), B, H, W, C, k, _stream()),
          "rpo_avgpool_nhwc")
    return y


def attnpool_tokens(x, pos, tokens):
    """[mean | pixels] + positional embedding (rpo_attnpool_tokens): x [B,H,W,C], pos fp32 [HW+1, C], tokens [B, HW+1, C]."""
    _nhwc(x, "x")
    B, H, W, C = x.shape
    assert pos.dtype == torch.float32 and pos.is_contiguous() and tuple(pos.shape) == (H * W + 1, C)
    assert tokens.is_contiguous() and tuple(tokens.shape) == (B, H * W + 1, C) and tokens.dtype == x.dtype
    check(_lib.load().rpo_attnpool_tokens(x.data_ptr(), pos.data_ptr(), tokens.data_ptr(), dtype_code(x.dtype), B, H * W, C,
                                          _stream()), "rpo_attnpool_tokens")
    return tokens


def attnpool_attn(q, kv, out, heads: int, scale: float):
    """The attention pool's query (rpo_attnpool_attn): q fp32 [B, C] (row stride free), kv [B, T, 2C], out [B, C]."""
    B, T, C2 = kv.shape
    C = C2 // 2
    assert q.dtype == torch.float32 and q.dim() == 2 and q.stride(1) == 1 and tuple(q.shape) == (B, C)
    assert kv.is_contiguous() and out.is_contiguous() and tuple(out.shape) == (B, C) and out.dtype == kv.dtype
    check(_lib.load().rpo_attnpool_attn(q.data_ptr(), q.stride(0), kv.data_ptr(), out.data_ptr(), dtype_code(kv.dtype), B, T,
                                        C, heads, scale, _stream()), "rpo_attnpool_attn")
    return out
