"""Fused top-k / top-p / temperature sampling of one token per row of logits (``csrc/kernels/sample.hip``).

One launch, device operations only: the random draw is a counter-based hash of ``(seed, step, row)`` and ``step`` is
read on the device, so a captured decode step draws a fresh number at every graph replay and the eager loop draws
the same ones.  Semantics (the reference composition ``sample_temperature(top_p_transform(top_k_transform(x, k), p),
T)`` with ties resolved by value, so nothing depends on a sort order):

* top-k (``k <= 0`` or ``k >= V``: off): keep logits ``>=`` the k-th largest (tie-mates of the k-th value are kept,
  as with the reference's ``logits < kth``);
* top-p (``p >= 1``: off) over what top-k kept: softmax at temperature 1; walking the distinct logit values
  downwards, the cut is the first value whose inclusive cumulative mass exceeds ``p`` (the token the reference's
  right shift still keeps); every logit ``>=`` cut is kept, the maximum always.  **Deviation from the reference**:
  the reference keeps a sort-order-dependent subset of the tokens tied with the cut token, this keeps all of them,
  a superset by at most those tie-mates;
* draw: softmax of ``logit / T`` over the kept set (row maximum subtracted before every exponential), inverse CDF in
  token-index order: the first kept index whose inclusive cumulative probability exceeds ``u``.  ``-inf`` (and NaN)
  logits have probability 0 and are never returned; a row without any finite logit returns token 0.

GPU tensors go to the HIP kernel (and raise without the extension); CPU tensors run :func:`sample_distribution`, a
float64 torch implementation of exactly these semantics that is also the numerical oracle of the GPU tests.
"""
from __future__ import annotations

from typing import Union

import torch

from ._ext import ext, use_native
from .attention import _M32, _mix32, _mul32


def _seed32(seed: int) -> int:
    seed = int(seed)
    return (seed ^ (seed >> 32)) & _M32


def sample_uniform(seed: int, step: Union[int, torch.Tensor], row: Union[int, torch.Tensor]) -> torch.Tensor:
    """The uniform in [0, 1) the kernel uses for (seed, step, row), as float64 (24 bits, exact); ``step`` and ``row``
    broadcast.  Same hash chain as ``sample.hip``: mix(mix(mix(mix(seed + 0x9e3779b9) ^ step_lo) + step_hi) ^
    row * 0x85ebca6b) >> 8, scaled by 2^-24."""
    step = torch.as_tensor(step, dtype=torch.long)
    row = torch.as_tensor(row, dtype=torch.long).to(step.device)
    h = _mix32(torch.tensor((_seed32(seed) + 0x9E3779B9) & _M32, dtype=torch.long, device=step.device))
    h = _mix32(h ^ (step & _M32))
    h = _mix32((h + ((step >> 32) & _M32)) & _M32)
    h = _mix32(h ^ _mul32(row & _M32, 0x85EBCA6B))
    return (h >> 8).double() / 16777216.0


def sample_distribution(logits: torch.Tensor, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0
                        ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """float64 reference of the filters and the draw distribution for ``logits [B, V]``: the kept mask ``[B, V]``, the
    inclusive CDF in token-index order ``[B, V]`` (all zeros for a row without a finite logit) and the cut logit
    ``[B]`` (``-inf`` when no filter is active)."""
    assert logits.dim() == 2 and temperature > 0
    x = logits.detach().float().double()  # the kernel works on the fp32 image of every dtype
    x = torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x) + 0.0  # -0 -> +0: ties are by value
    B, V = x.shape
    p = float(torch.tensor(top_p, dtype=torch.float32))  # the kernel receives fp32
    inv_t = float(1.0 / torch.tensor(temperature, dtype=torch.float32))
    m = x.max(dim=-1, keepdim=True).values
    dead = torch.isinf(m) & (m < 0)
    m = torch.where(dead, torch.zeros_like(m), m)
    cut = torch.full((B, 1), float("-inf"), dtype=torch.float64, device=x.device)
    if 0 < top_k < V:
        cut = torch.topk(x, top_k, dim=-1).values[:, -1:]
    if p < 1.0:
        e = torch.where(x >= cut, torch.exp(x - m), torch.zeros_like(x))
        xs, order = torch.sort(x, dim=-1, descending=True)
        cum = torch.cumsum(torch.gather(e, 1, order), dim=-1)
        over = cum > max(p, 0.0) * e.sum(dim=-1, keepdim=True)
        first = torch.where(over.any(dim=-1), over.to(torch.uint8).argmax(dim=-1), torch.zeros(B, dtype=torch.long, device=x.device))
        cut = torch.maximum(cut, torch.gather(xs, 1, first[:, None]))
    kept = (x >= cut) & ~torch.isinf(x) & ~dead
    w = torch.where(kept, torch.exp((x - m) * inv_t), torch.zeros_like(x))
    tot = w.sum(dim=-1, keepdim=True)
    cdf = torch.cumsum(w, dim=-1) / torch.where(tot > 0, tot, torch.ones_like(tot))
    return kept, cdf, cut[:, 0]


def _sample_torch(logits: torch.Tensor, step: torch.Tensor, seed: int, temperature: float, top_k: int, top_p: float,
                  want_info: bool):
    kept, cdf, cut = sample_distribution(logits, temperature, top_k, top_p)
    B, V = kept.shape
    u = sample_uniform(seed, step.reshape(()), torch.arange(B, device=logits.device))
    hit = kept & (cdf > u[:, None])
    idx = torch.arange(V, device=logits.device)
    last = torch.where(kept, idx, torch.zeros_like(idx)).max(dim=-1).values  # the CDF's rounding at the upper edge
    tokens = torch.where(hit.any(dim=-1), hit.to(torch.uint8).argmax(dim=-1), last)
    if not want_info:
        return tokens
    info = torch.stack([kept.sum(dim=-1).to(torch.int32), cut.float().view(torch.int32)], dim=-1)
    return tokens, info


def sample_logits(logits: torch.Tensor, step: Union[int, torch.Tensor], seed: int, temperature: float = 1.0,
                  top_k: int = 0, top_p: float = 1.0, want_info: bool = False):
    """One token per row of ``logits [B, V]`` (bf16 / fp16 / fp32, unit last stride, any row stride): ``tokens [B]``
    int64, with ``want_info`` also ``info [B, 2]`` int32 = (number of tokens kept by both filters, bits of the fp32 cut
    logit).  ``step`` is one int64 (a tensor on the logits' device stays on the device: no host sync)."""
    if logits.dim() != 2:
        raise ValueError(f"sample_logits: logits must be [B, V], got {tuple(logits.shape)}")
    if not temperature > 0:
        raise ValueError("sample_logits: temperature must be positive")
    if not torch.is_tensor(step):
        step = torch.tensor([int(step)], dtype=torch.long, device=logits.device)
    if step.dtype != torch.long or step.numel() != 1 or step.device != logits.device:
        raise ValueError("sample_logits: step must be one int64 on the logits' device")
    if use_native(logits):
        out = ext().sample_logits(logits, step, _seed32(seed), float(temperature), int(top_k), float(top_p), want_info)
        return (out[0], out[1]) if want_info else out[0]
    return _sample_torch(logits, step, seed, float(temperature), int(top_k), float(top_p), want_info)
