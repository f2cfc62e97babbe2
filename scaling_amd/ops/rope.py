"""Rotary position embedding (both conventions) with a HIP kernel (``csrc/kernels/swiglu_rope.hip``).

Inputs are token-major ``[T, heads, head_dim]`` views — typically strided slices of the fused QKV
GEMM output — and the kernel writes a contiguous rotated copy, so the attention kernel reads packed
heads.  Tables are fp32 ``[max_pos, rot_dim/2]``; the NeoX (rotate-half) table holds the cos/sin
values rounded through the model dtype, matching the reference's buffers (``rotary.py:93-108``);
the complex/interleaved table is fp32 as in ``rotary.py:45-90``.
"""
from __future__ import annotations

from typing import Any, Optional

import torch

from ._ext import ext, use_native


def rope_tables(dim: int, max_pos: int, base: float, interleaved: bool, dtype: torch.dtype, device: Any):
    inv_freq = 1.0 / (float(base) ** (torch.arange(0, dim, 2).float() / dim))
    t = torch.arange(max_pos).float()
    freqs = torch.outer(t, inv_freq)
    cos, sin = freqs.cos(), freqs.sin()
    if not interleaved and dtype != torch.float32:
        cos, sin = cos.to(dtype).float(), sin.to(dtype).float()
    return cos.contiguous().to(device), sin.contiguous().to(device)


def rope_reference(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: Optional[torch.Tensor],
                   rot_dim: int, seq_len: int, interleaved: bool) -> torch.Tensor:
    T = x.shape[0]
    p = pos.reshape(-1).long() if pos is not None else torch.arange(T, device=x.device) % seq_len
    c = cos[p][:, None, :]
    s = sin[p][:, None, :]
    xf = x.float()
    rot, rest = xf[..., :rot_dim], xf[..., rot_dim:]
    if interleaved:
        x0, x1 = rot[..., 0::2], rot[..., 1::2]
        o0, o1 = x0 * c - x1 * s, x1 * c + x0 * s
        out = torch.stack([o0, o1], dim=-1).flatten(-2)
    else:
        h = rot_dim // 2
        x0, x1 = rot[..., :h], rot[..., h:]
        out = torch.cat([x0 * c - x1 * s, x1 * c + x0 * s], dim=-1)
    return torch.cat([out, rest], dim=-1).to(x.dtype)


def rope_kv_write_chunk(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, cu_q: torch.Tensor, start: torch.Tensor,
                        table: torch.Tensor, page: int, nq: int, nkv: int, rot_dim: int, interleaved: bool,
                        kc: torch.Tensor, vc: torch.Tensor, err: torch.Tensor,
                        kv_scales: Optional[tuple[torch.Tensor, torch.Tensor]] = None) -> torch.Tensor:
    """RoPE + paged K/V write of a packed chunk pass (``csrc/kernels/swiglu_rope.hip``, one launch on the GPU).

    x ``[T, nq + 2 nkv, hd]`` is the pass's projection (heads q | k | v, contiguous); tokens ``cu_q[s] .. cu_q[s + 1]``
    (int32 ``[nseg + 1]``) form segment s and token t sits at position ``p = start[s] + t - cu_q[s]`` (``start`` int64
    ``[nseg]``).  Returns the rotated q ``[T, nq, hd]``; the rotated k and v go to row ``table[s, p // page] * page +
    p % page`` of the pools kc / vc ``[num_pages * page, nkv, hd]`` (``table`` int32 ``[nseg, max_pages]``).  With
    ``kv_scales`` = (k_scale, v_scale) float32 ``[nkv, pool rows]`` the pools hold e4m3 codes and every (token, head) row
    is quantised as the one-token append does (bfloat16 x only).  A token whose position is outside ``[0, min(max_pages
    * page, rotary rows))`` or whose table entry is outside the pool writes nothing, gets zero q rows and sets bit 0 of
    ``err``; bit 1: a non-finite k / v value was replaced (FP8).  On the GPU every token is bitwise what
    ``ext().rope_kv_append_paged`` writes for one token at p; operands the kernel does not take raise ``ValueError``.
    ``cu_q[nseg]`` must be T (q rows past the last segment are not written).
    CPU tensors run the unfused composition (rotation, then indexed row writes)."""
    sc = kv_scales if kv_scales is not None else (None, None)
    if use_native(x):
        q = ext().rope_kv_write_chunk(x, cos, sin, cu_q, start, nq, nkv, rot_dim, interleaved, kc, vc, err, table,
                                      int(page), sc[0], sc[1])
        if q is None:
            raise ValueError(f"rope_kv_write_chunk: no kernel for x {tuple(x.shape)} {x.dtype}, rot_dim {rot_dim}, "
                             f"pool {kc.dtype} (contiguous bf16 / fp16 x with head dim % 8 == 0 and <= 512, rot_dim % "
                             "16 == 0 (% 8 interleaved), bf16 x for an FP8 pool)")
        return q
    from .quant import quantize_kv_rows, sanitize_kv

    cu = cu_q.long()
    seg = torch.repeat_interleave(torch.arange(start.numel()), cu[1:] - cu[:-1])
    pos = start.long()[seg] + torch.arange(x.shape[0]) - cu[seg]
    ok = (pos >= 0) & (pos < min(table.shape[1] * page, cos.shape[0]))
    p = pos * ok
    entry = table.long()[seg, p // page]
    ok &= (entry >= 0) & (entry < kc.shape[0] // page)
    p = p * ok
    q = apply_rope(x[:, :nq], cos, sin, p, rot_dim, 1, interleaved) * ok.view(-1, 1, 1).to(x.dtype)
    k = apply_rope(x[:, nq : nq + nkv], cos, sin, p, rot_dim, 1, interleaved)
    rows = (entry * page + p % page)[ok]
    for pool, scale, val in ((kc, sc[0], k[ok]), (vc, sc[1], x[:, nq + nkv :][ok])):  # PagedKVCache[FP8].write_rows' ops
        if scale is not None:
            val, nonfinite = sanitize_kv(val)
            val, s = quantize_kv_rows(val, check=False)
            scale.index_copy_(1, rows, s)
            err.bitwise_or_(nonfinite.to(torch.int32) * 2)
        pool.index_copy_(0, rows, val.to(pool.dtype))
    err.bitwise_or_((~ok).any().to(torch.int32))
    return q


class _Rope(torch.autograd.Function):
    @staticmethod
    def forward(ctx: Any, x, cos, sin, pos, rot_dim, seq_len, interleaved):  # type: ignore[override]
        ctx.save_for_backward(cos, sin, pos)
        ctx.cfg = (rot_dim, seq_len, interleaved)
        return ext().rope(x, cos, sin, pos, rot_dim, seq_len, interleaved, False)

    @staticmethod
    def backward(ctx: Any, dy: torch.Tensor):  # type: ignore[override]
        cos, sin, pos = ctx.saved_tensors
        rot_dim, seq_len, interleaved = ctx.cfg
        dx = ext().rope(dy.contiguous(), cos, sin, pos, rot_dim, seq_len, interleaved, True)
        return dx, None, None, None, None, None, None


def apply_rope(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: Optional[torch.Tensor], rot_dim: int,
               seq_len: int, interleaved: bool) -> torch.Tensor:
    """x: [T, heads, head_dim]; pos: [T] absolute positions or None (position = t % seq_len)."""
    if use_native(x):
        if pos is not None:
            pos = pos.reshape(-1).long().contiguous()
        return _Rope.apply(x, cos, sin, pos, rot_dim, seq_len, interleaved)
    return rope_reference(x, cos, sin, pos, rot_dim, seq_len, interleaved)
