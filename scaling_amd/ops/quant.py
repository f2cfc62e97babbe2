"""FP8 weight-only quantisation for token-by-token decoding (the FP8 weight format of ``csrc/kernels/gemv.hip``).

Scheme ``fp8_e4m3``: one output row of ``W [N, K]`` at a time.

* codes: OCP ``e4m3fn`` (``torch.float8_e4m3fn``; not the ``fnuz`` variant), one byte per weight;
* scale: one fp32 **power of two** per row, ``s = 2^ceil(log2(amax / 448))`` so that ``amax / s`` lies in
  ``(224, 448]`` (``s = 1`` for an all-zero row);
* ``q = cast_e4m3(clamp(w / s, -448, 448))``, round to nearest even in fp32; the NaN codes are never produced and
  non-finite input is refused.

Because the scale is a power of two, ``q * s`` is exactly representable in bf16 (a code has 4 significant bits, bf16
has 8): the FP8 copy is an exact encoding of a bf16 matrix.  ``quantize_parameters`` therefore overwrites the bf16
parameter with the dequantised values, and every path that does not stream the FP8 copy -- prefill GEMMs, CPU, any
fallback -- computes the same function from the same weights.

The copy hangs on the parameter as ``_sa_w8 = (q, scale, version)``; ``version`` is the parameter's ``_version`` right
after the dequantised values were written back.  Any later in-place change of the parameter (checkpoint load,
optimizer step, LoRA merge) moves ``_version``: the copy is then dropped with a one-time warning and the bf16 path
serves the layer.  A stale copy is never used.

Scheme ``mxfp4`` (OCP MXFP4, the third weight format of ``gemv.hip`` / ``skinny.hip``): blocks of 32 consecutive k of
one row.

* codes: OCP ``e2m1`` -- a sign bit and one of ``{0, 0.5, 1, 1.5, 2, 3, 4, 6}`` --, two per byte: weight ``2i`` in the
  low nibble and weight ``2i + 1`` in the high nibble (``uint8 [N, K / 2]``; the order of ``torch.float4_e2m1fn_x2``
  and of ``v_cvt_scalef32_pk_*_fp4``); ``-0`` is never produced and decodes as 0;
* scale: one ``e8m0`` byte ``b`` per block, value ``2^(b - 127)`` (``uint8 [N, K / 32]``): the FP8 rule per block,
  ``s = 2^ceil(log2(amax / 6))``, so ``amax / s`` lies in ``(3, 6]`` and nothing saturates (``s = 1`` for an all-zero
  block, the exponent clamped below at ``_MIN_EXP``; the NaN byte 255 is never produced);
* rounding of ``|w| / s`` to the nearest code, ties to the even code.

A code has 2 significant bits and the scale is a power of two, so ``code * s`` is again exactly a bf16 number and
everything above holds: the parameter is overwritten with the dequantised values and the copy hangs on it as
``_sa_w4 = (codes, scales, version)`` under the same staleness rule.  A parameter carries at most one copy.
``wq_of`` / ``adjacent_wq`` are the format-agnostic lookups of the decode call sites: they yield the binding suffix
(``"_w8"`` or ``"_w4"``) together with the copy.
"""
from __future__ import annotations

import warnings
from typing import Optional, Sequence

import torch

FP8_MAX = 448.0
SCHEME = "fp8_e4m3"
PIECE = 16  # weights per 16-byte piece of the GEMV kernel: K must be a multiple
_ATTR = "_sa_w8"
SCHEME_MXFP4 = "mxfp4"
SCHEMES = (SCHEME, SCHEME_MXFP4)
MX_BLOCK = 32  # weights per MXFP4 block (= per 16-byte piece of codes): K must be a multiple
FP4_MAX = 6.0
MX_AMAX_LIMIT = 2.0 ** 120  # above, a block near the top of the bf16 range could round to an infinite value
_ATTR4 = "_sa_w4"
_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
_MIN_EXP = -100  # smallest row-scale exponent: q * s stays a normal bf16 / fp32 number down to the subnormal codes
_warned = [False]


def quantize_rows_fp8(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """``(q [N, K] float8_e4m3fn, scale [N] fp32)`` of a 2-D matrix, one power-of-two scale per row."""
    if w.dim() != 2:
        raise ValueError(f"quantize_rows_fp8: expected a 2-D weight, got shape {tuple(w.shape)}")
    wf = w.detach().float()
    if not bool(torch.isfinite(wf).all()):
        raise ValueError("quantize_rows_fp8: the weight holds non-finite values")
    return _quantize_rows(wf)


def _quantize_rows(wf: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """The arithmetic of ``quantize_rows_fp8`` on a finite fp32 matrix (device ops only, no host read)."""
    amax = wf.abs().amax(dim=1) if wf.shape[1] > 0 else wf.new_zeros(wf.shape[0])
    zero = amax == 0
    # amax / 448 = m * 2^e with m in [0.5, 1): ceil(log2) is e, or e - 1 when m is exactly 0.5
    m, e = torch.frexp(torch.where(zero, torch.full_like(amax, FP8_MAX), amax) / FP8_MAX)
    e = torch.where(m == 0.5, e - 1, e).clamp_(min=_MIN_EXP)
    one = torch.ones_like(amax)
    s = torch.ldexp(one, e)
    # guard the rounding of the division: amax <= 448 s must hold, and must fail for s / 2 (both products are exact)
    s = torch.where(amax > FP8_MAX * s, s * 2, s)
    s = torch.where((amax <= (FP8_MAX / 2) * s) & (torch.ldexp(one, torch.full_like(e, _MIN_EXP)) < s), s / 2, s)
    s = torch.where(zero, one, s)
    q = (wf / s[:, None]).clamp_(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn)
    return q, s


def dequantize_rows_fp8(q: torch.Tensor, scale: torch.Tensor, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """``q * scale[:, None]`` in ``dtype`` (exact in bf16 and fp32 for the scales ``quantize_rows_fp8`` makes)."""
    if q.dtype == torch.uint8:
        q = q.view(torch.float8_e4m3fn)
    return (q.float() * scale.float()[:, None]).to(dtype)


# The largest K/V magnitude the cache format takes.  A row with amax in (240 * 2^120, bf16 max] would round amax to the
# code of 256 at scale 2^120, and 256 * 2^120 = 2^128 is infinite in bf16; the cut sits at the power of two below.
KV_MAX = 2.0 ** 127


def quantize_kv_rows(x: torch.Tensor, check: bool = True) -> tuple[torch.Tensor, torch.Tensor]:
    """K or V cache rows ``x [rows, nkv, hd]`` in the FP8 cache format: ``(codes [rows, nkv, hd] uint8, scale
    [nkv, rows] fp32)``.  A row of the format is one token of one kv head: its codes and scale are exactly
    ``quantize_rows_fp8`` of that row viewed as ``[1, hd]`` (e4m3fn codes, one power-of-two scale).  The scales are
    head-major, the layout of the cache and of the decode kernel.  Works on CPU and GPU tensors.

    ``check=False`` skips the finiteness test (a host read): the caller has replaced non-finite values."""
    if x.dim() != 3:
        raise ValueError(f"quantize_kv_rows: expected [rows, nkv, hd], got shape {tuple(x.shape)}")
    rows, nkv, hd = x.shape
    flat = x.detach().reshape(rows * nkv, hd)
    q, s = quantize_rows_fp8(flat) if check else _quantize_rows(flat.float())
    return q.view(torch.uint8).view(rows, nkv, hd), s.view(rows, nkv).t().contiguous()


def dequantize_kv_rows(codes: torch.Tensor, scale: torch.Tensor, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """``[rows, nkv, hd]`` values of ``quantize_kv_rows`` output (codes uint8 or float8_e4m3fn, scale ``[nkv, rows]``);
    exact in bf16 and fp32."""
    if codes.dim() != 3 or tuple(scale.shape) != (codes.shape[1], codes.shape[0]):
        raise ValueError(f"dequantize_kv_rows: codes {tuple(codes.shape)} need scales [nkv, rows], got {tuple(scale.shape)}")
    rows, nkv, hd = codes.shape
    flat = dequantize_rows_fp8(codes.reshape(rows * nkv, hd), scale.t().reshape(rows * nkv), dtype)
    return flat.view(rows, nkv, hd)


def sanitize_kv(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """``x`` as bf16 with NaN -> 0 and every magnitude above ``KV_MAX`` (2^127; infinity included) -> +-2^127 -- what
    the FP8 append kernel stores, so that the largest code times the row's scale stays finite --, and a 0-d bool
    tensor: whether anything was replaced.  Device ops only."""
    xb = x.detach().to(torch.bfloat16)
    nan = torch.isnan(xb)
    big = xb.abs() > KV_MAX
    xb = torch.where(nan, torch.zeros_like(xb), xb.clamp(-KV_MAX, KV_MAX))
    return xb, (nan | big).any()


def attach_w8(param: torch.Tensor, q: torch.Tensor, scale: torch.Tensor) -> None:
    """Hangs the FP8 copy on ``param``; call right after the dequantised values were written into it."""
    setattr(param, _ATTR, (q, scale, param._version))


def drop_w8(param: torch.Tensor) -> None:
    if hasattr(param, _ATTR):
        delattr(param, _ATTR)


def _valid_copy(param: torch.Tensor, attr: str, name: str, stacklevel: int
                ) -> Optional[tuple[torch.Tensor, torch.Tensor]]:
    c = getattr(param, attr, None)
    if c is None:
        return None
    shape = param.shape if attr == _ATTR else (param.shape[0], param.shape[1] // 2)
    if c[2] != param._version or c[0].shape != shape or c[0].device != param.device:
        delattr(param, attr)
        if not _warned[0]:
            _warned[0] = True
            warnings.warn(f"scaling_amd: a quantised weight was modified after quantize_weights(); its {name} copy is "
                          "dropped and the layer runs from the bf16 parameter (call quantize_weights() again to "
                          "re-quantise)", RuntimeWarning, stacklevel=stacklevel)
        return None
    return c[0], c[1]


def w8_of(param: torch.Tensor) -> Optional[tuple[torch.Tensor, torch.Tensor]]:
    """The valid FP8 copy ``(q, scale)`` of ``param``, or None.  A copy whose parameter changed in place since it
    was made is dropped (one warning per process) and None is returned: the caller takes the bf16 path."""
    return _valid_copy(param, _ATTR, "FP8", 3)


def attach_w4(param: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor) -> None:
    """Hangs the MXFP4 copy on ``param``; call right after the dequantised values were written into it."""
    setattr(param, _ATTR4, (codes, scales, param._version))


def drop_w4(param: torch.Tensor) -> None:
    if hasattr(param, _ATTR4):
        delattr(param, _ATTR4)


def w4_of(param: torch.Tensor) -> Optional[tuple[torch.Tensor, torch.Tensor]]:
    """The valid MXFP4 copy ``(codes, scales)`` of ``param``, or None; staleness as ``w8_of``."""
    return _valid_copy(param, _ATTR4, "MXFP4", 3)


def has_copy(param: torch.Tensor) -> bool:
    """Whether a quantised copy of either format hangs on ``param`` (valid or not: a cheap attribute test)."""
    return getattr(param, _ATTR, None) is not None or getattr(param, _ATTR4, None) is not None


def wq_of(param: torch.Tensor) -> Optional[tuple[str, torch.Tensor, torch.Tensor]]:
    """``(suffix, copy, scales)`` of the valid quantised copy of ``param`` -- ``("_w8", q, scale)`` or
    ``("_w4", codes, scales)``; the suffix names the bindings that take the copy -- or None."""
    c = w8_of(param)
    if c is not None:
        return "_w8", c[0], c[1]
    c = w4_of(param)
    return None if c is None else ("_w4", c[0], c[1])


def adjacent_w8(weights: Sequence[torch.Tensor]) -> Optional[tuple[torch.Tensor, torch.Tensor]]:
    """The fused ``(q [sum N, K], scale [sum N])`` view over the valid copies of weights that were quantised as one
    group (their copies are row slices of one buffer, back to back); None otherwise."""
    cs = [w8_of(w) for w in weights]  # (every member is checked, so every stale copy is dropped)
    if any(c is None for c in cs):
        return None
    if len(cs) == 1:
        return cs[0] if cs[0][0].is_contiguous() else None  # type: ignore[index]
    q0, s0 = cs[0]  # type: ignore[misc]
    K = q0.shape[1]
    qn, sn, rows = q0.data_ptr(), s0.data_ptr(), 0
    for q, s in cs:  # type: ignore[misc]
        if not (q.is_contiguous() and s.is_contiguous() and q.shape[1] == K and q.dtype == q0.dtype
                and q.data_ptr() == qn and s.data_ptr() == sn
                and q.untyped_storage().data_ptr() == q0.untyped_storage().data_ptr()
                and s.untyped_storage().data_ptr() == s0.untyped_storage().data_ptr()):
            return None
        qn += q.numel() * q.element_size()
        sn += s.numel() * s.element_size()
        rows += q.shape[0]
    return torch.as_strided(q0, (rows, K), (K, 1)), torch.as_strided(s0, (rows,), (1,))


def adjacent_w4(weights: Sequence[torch.Tensor]) -> Optional[tuple[torch.Tensor, torch.Tensor]]:
    """``adjacent_w8`` for MXFP4 copies: the fused ``(codes [sum N, K / 2], scales [sum N, K / 32])`` view."""
    cs = [w4_of(w) for w in weights]  # (every member is checked, so every stale copy is dropped)
    if any(c is None for c in cs):
        return None
    if len(cs) == 1:
        return cs[0] if cs[0][0].is_contiguous() and cs[0][1].is_contiguous() else None  # type: ignore[index]
    q0, s0 = cs[0]  # type: ignore[misc]
    KB, KS = q0.shape[1], s0.shape[1]
    qn, sn, rows = q0.data_ptr(), s0.data_ptr(), 0
    for q, s in cs:  # type: ignore[misc]
        if not (q.is_contiguous() and s.is_contiguous() and q.shape[1] == KB and s.shape[1] == KS
                and q.data_ptr() == qn and s.data_ptr() == sn
                and q.untyped_storage().data_ptr() == q0.untyped_storage().data_ptr()
                and s.untyped_storage().data_ptr() == s0.untyped_storage().data_ptr()):
            return None
        qn += q.numel()
        sn += s.numel()
        rows += q.shape[0]
    return torch.as_strided(q0, (rows, KB), (KB, 1)), torch.as_strided(s0, (rows, KS), (KS, 1))


def adjacent_wq(weights: Sequence[torch.Tensor]) -> Optional[tuple[str, torch.Tensor, torch.Tensor]]:
    """The fused copy of weights quantised as one group, whichever format it has: ``(suffix, copy, scales)`` as
    ``wq_of``; None without a valid copy of every member in one format (stale copies are dropped on the way)."""
    c = adjacent_w8(weights)
    if c is not None:
        return "_w8", c[0], c[1]
    c = adjacent_w4(weights)
    return None if c is None else ("_w4", c[0], c[1])


def quantize_rows_mxfp4(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """``(codes [N, K / 2] uint8, scales [N, K / 32] uint8)`` of a 2-D matrix with ``K % 32 == 0``: e2m1 codes, two per
    byte (even k in the low nibble), one e8m0 scale byte per block of 32.  Works on CPU and GPU tensors."""
    if w.dim() != 2 or w.shape[1] % MX_BLOCK != 0:
        raise ValueError(f"quantize_rows_mxfp4: expected a 2-D weight with K a multiple of {MX_BLOCK}, got shape "
                         f"{tuple(w.shape)}")
    wf = w.detach().float()
    if not bool(torch.isfinite(wf).all()):
        raise ValueError("quantize_rows_mxfp4: the weight holds non-finite values")
    if wf.numel() and float(wf.abs().max()) > MX_AMAX_LIMIT:
        raise ValueError("quantize_rows_mxfp4: the weight holds magnitudes above 2^120")
    N, K = wf.shape
    blk = wf.view(N, K // MX_BLOCK, MX_BLOCK)
    amax = blk.abs().amax(dim=2) if K > 0 else wf.new_zeros(N, 0)
    zero = amax == 0
    # amax / 6 = m * 2^e with m in [0.5, 1): ceil(log2) is e, or e - 1 when m is exactly 0.5
    m, e = torch.frexp(torch.where(zero, torch.full_like(amax, FP4_MAX), amax) / FP4_MAX)
    e = torch.where(m == 0.5, e - 1, e).clamp_(min=_MIN_EXP)
    one = torch.ones_like(amax)
    s = torch.ldexp(one, e)
    # guard the rounding of the division: amax <= 6 s must hold, and must fail for s / 2 (both products are exact)
    s = torch.where(amax > FP4_MAX * s, s * 2, s)
    s = torch.where((amax <= (FP4_MAX / 2) * s) & (torch.ldexp(one, torch.full_like(e, _MIN_EXP)) < s), s / 2, s)
    s = torch.where(zero, one, s)
    a = (blk / s[:, :, None]).abs().reshape(N, K)  # exact: s is a power of two
    # nearest code, ties to the even code: a tie goes up at 0.75, 1.75, 3.5 and stays at 0.25, 1.25, 2.5, 5
    stay = torch.tensor([0.25, 1.25, 2.5, 5.0], device=a.device)
    up = torch.tensor([0.75, 1.75, 3.5], device=a.device)
    idx = torch.bucketize(a, stay, right=False) + torch.bucketize(a, up, right=True)
    code = (idx | (((wf < 0) & (idx > 0)).to(idx.dtype) << 3)).to(torch.uint8)  # no -0
    codes = code[:, 0::2] | (code[:, 1::2] << 4)
    scales = (torch.frexp(s)[1] - 1 + 127).to(torch.uint8)
    return codes.contiguous(), scales.contiguous()


def dequantize_rows_mxfp4(codes: torch.Tensor, scales: torch.Tensor, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """``[N, K]`` values of ``quantize_rows_mxfp4`` output; exact in bf16 and fp32.  The code ``-0`` decodes as 0."""
    if codes.dim() != 2 or scales.dim() != 2 or codes.shape[0] != scales.shape[0] or codes.shape[1] != 16 * scales.shape[1]:
        raise ValueError(f"dequantize_rows_mxfp4: codes {tuple(codes.shape)} need scales [N, K / 32], got {tuple(scales.shape)}")
    N = codes.shape[0]
    c = codes.view(torch.uint8) if codes.dtype != torch.uint8 else codes
    lut = torch.tensor(_E2M1 + tuple(-v for v in _E2M1), dtype=torch.float32, device=c.device)
    v = torch.stack([lut[(c & 15).long()], lut[(c >> 4).long()]], dim=2).view(N, -1, MX_BLOCK)
    s = torch.ldexp(torch.ones((), device=c.device), scales.to(torch.int32) - 127)
    return (v * s[:, :, None]).view(N, -1).to(dtype)


@torch.no_grad()
def quantize_parameters(weights: Sequence[torch.Tensor], scheme: str = SCHEME) -> tuple[int, int]:
    """Quantises a group of 2-D bf16 weights that share their input (one ``[sum N, K]`` buffer of codes and one
    ``[sum N]`` buffer of scales -- ``[sum N, K / 2]`` and ``[sum N, K / 32]`` for ``mxfp4`` --; each member's copy is
    a row slice), overwrites each weight with its dequantised values and attaches the copies; a copy of the other
    format is dropped.  Returns ``(bf16 bytes, bytes of the copy incl. scales)``."""
    if scheme not in SCHEMES:
        raise ValueError(f"quantize_parameters: unknown scheme {scheme!r} (supported: {', '.join(map(repr, SCHEMES))})")
    for w in weights:
        if w.dim() != 2 or w.dtype != torch.bfloat16:
            raise ValueError("quantize_parameters: 2-D bfloat16 weights only")
    if scheme == SCHEME_MXFP4:
        codes, scales = quantize_rows_mxfp4(torch.cat([w.detach() for w in weights], dim=0) if len(weights) > 1 else weights[0].detach())
        deq = dequantize_rows_mxfp4(codes, scales, torch.bfloat16)
        off = 0
        for w in weights:
            n = w.shape[0]
            w.copy_(deq[off : off + n])
            drop_w8(w)
            attach_w4(w, codes[off : off + n], scales[off : off + n])
            off += n
        return deq.numel() * 2, codes.numel() + scales.numel()
    q, s = quantize_rows_fp8(torch.cat([w.detach() for w in weights], dim=0) if len(weights) > 1 else weights[0].detach())
    q, s = q.contiguous(), s.contiguous()
    deq = dequantize_rows_fp8(q, s, torch.bfloat16)
    off = 0
    for w in weights:
        n = w.shape[0]
        w.copy_(deq[off : off + n])
        drop_w4(w)
        attach_w8(w, q[off : off + n], s[off : off + n])
        off += n
    return deq.numel() * 2, q.numel() + s.numel() * 4
