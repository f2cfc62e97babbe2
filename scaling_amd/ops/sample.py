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

from typing import Optional, Union

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


# ---------------------------------------------------------------------------------------------------------------------
# Row-table form: per-row parameters, penalties and history (``sample_rows_kernel`` in ``csrc/kernels/sample.hip``)
_COLUMNS = (("active", torch.int32), ("temperature", torch.float32), ("top_k", torch.int32), ("top_p", torch.float32),
            ("seed", torch.int32), ("step", torch.int64), ("rep", torch.float32), ("inv_rep", torch.float32),
            ("presence", torch.float32), ("hist_len", torch.int32))
_HEADER = 12  # int32 words of one row's scalars in front of its history: step (two words, 8-byte aligned) comes first
_OFFSETS = {"step": 0, **{name: 2 + i for i, name in enumerate(n for n, _ in _COLUMNS if n != "step")}}


class RowTable:
    """The sampler's table for B decoder rows, a struct of arrays at fixed addresses: ``active`` (int32; 0: the row
    draws nothing and changes nothing), ``temperature`` (fp32; 0 is greedy), ``top_k`` / ``top_p`` (int32 / fp32),
    ``seed`` (int32 holding the request's 32 seed bits), ``step`` (int64, the request's own draw counter), ``rep`` /
    ``inv_rep`` / ``presence`` (fp32; ``inv_rep`` = fp32(1 / rep)), ``hist_len`` (int32) and ``hist`` ``[B, H]`` int32
    (the request's own tokens).  ``rows(a, b)`` is the table of rows ``a .. b - 1`` over the same memory.

    ``RowTable.empty`` lays one row's scalars and history out contiguously in one int32 buffer ``buf [B, 12 + H]`` (the
    columns are strided views of it), so that a host fills a row with one copy."""

    def __init__(self, hist: torch.Tensor, buf: Optional[torch.Tensor] = None, **columns: torch.Tensor) -> None:
        self.hist, self.buf = hist, buf
        for name, _ in _COLUMNS:
            setattr(self, name, columns[name])

    @classmethod
    def empty(cls, rows: int, history: int, device: Union[None, str, torch.device] = None) -> "RowTable":
        if rows < 1 or history < 1:
            raise ValueError("RowTable: rows and history must be at least 1")
        width = _HEADER + history + (history & 1)  # even: the int64 step column stays 8-byte aligned
        buf = torch.zeros(rows, width, dtype=torch.int32, device=device)
        cols = {}
        for name, dtype in _COLUMNS:
            at = _OFFSETS[name]
            cols[name] = buf[:, at : at + (2 if dtype == torch.int64 else 1)].view(dtype)[:, 0]
        table = cls(buf[:, _HEADER : _HEADER + history], buf, **cols)
        table.temperature.fill_(1.0)
        table.top_p.fill_(1.0)
        table.rep.fill_(1.0)
        table.inv_rep.fill_(1.0)
        return table

    @property
    def columns(self) -> list[torch.Tensor]:
        return [getattr(self, name) for name, _ in _COLUMNS]

    def rows(self, start: int, stop: int) -> "RowTable":
        return RowTable(self.hist[start:stop], None if self.buf is None else self.buf[start:stop],
                        **{name: getattr(self, name)[start:stop] for name, _ in _COLUMNS})


def _check_table(logits: torch.Tensor, table: RowTable) -> None:
    B = logits.shape[0]
    for (name, dtype), col in zip(_COLUMNS, table.columns):
        if col.dtype != dtype or col.device != logits.device or col.dim() != 1 or col.shape[0] < B:
            raise ValueError(f"sample_rows: column {name} must be {dtype} with at least {B} entries on the logits' device")
    h = table.hist
    if h.dtype != torch.int32 or h.device != logits.device or h.dim() != 2 or h.shape[0] < B:
        raise ValueError(f"sample_rows: hist must be int32 [>= {B}, H] on the logits' device")
    if h.shape[1] > 1 and h.stride(1) != 1:
        raise ValueError("sample_rows: hist needs a unit stride along H")


def _penalised(x: torch.Tensor, seen: torch.Tensor, rep: torch.Tensor, inv_rep: torch.Tensor, presence: torch.Tensor
               ) -> torch.Tensor:
    """The penalised fp32 image of one row ``x [V]`` (fp32, NaN already -inf): a seen token's logit becomes
    ``(x > 0 ? x * inv_rep : x * rep) - presence`` in two separately rounded fp32 operations."""
    y = torch.where(x > 0, x * inv_rep, x * rep) - presence
    y = torch.where(torch.isnan(y), torch.full_like(y, float("-inf")), y) + 0.0
    return torch.where(seen, y, x)


def sample_rows_reference(logits: torch.Tensor, table: RowTable
                          ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """float64 twin of the row-table kernel's filters and distribution for ``logits [B, V]``; reads the table, changes
    nothing.  Per row: the kept mask ``[B, V]``, the inclusive CDF in token-index order ``[B, V]``, the cut ``[B]`` and
    the penalised fp32 row ``[B, V]``.  The two penalty roundings are done in fp32 and only then widened, so kept sets
    and cuts are exact.  A greedy row (temperature 0) keeps the maxima of its penalised row, its cut is the maximum; an
    inactive row keeps nothing."""
    assert logits.dim() == 2
    B, V = logits.shape
    x = logits.detach().float()
    x = torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x) + 0.0
    kept = torch.zeros(B, V, dtype=torch.bool, device=x.device)
    cdf = torch.zeros(B, V, dtype=torch.float64, device=x.device)
    cut = torch.full((B,), float("-inf"), dtype=torch.float64, device=x.device)
    pen = x.clone()
    ids = torch.arange(V, device=x.device)
    for b in range(B):
        if int(table.active[b]) == 0:
            continue
        rep, presence = table.rep[b], table.presence[b]
        if float(rep) != 1.0 or float(presence) != 0.0:
            n = min(max(int(table.hist_len[b]), 0), table.hist.shape[1])
            seen = torch.isin(ids, table.hist[b, :n].long())
            pen[b] = _penalised(x[b], seen, rep, table.inv_rep[b], presence)
        row = pen[b : b + 1]
        temperature = float(table.temperature[b])
        if temperature == 0.0:
            m = row.max()
            k = (row[0] == m) & ~torch.isinf(m)
            kept[b], cut[b] = k, m.double()
            cdf[b] = torch.cumsum(k.double(), 0) / max(int(k.sum()), 1)
        else:
            k, c, ct = sample_distribution(row, temperature, int(table.top_k[b]), float(table.top_p[b]))
            kept[b], cdf[b], cut[b] = k[0], c[0], ct[0]
    return kept, cdf, cut, pen


def _sample_rows_torch(logits: torch.Tensor, table: RowTable, info: Optional[torch.Tensor]) -> torch.Tensor:
    kept, cdf, cut, _ = sample_rows_reference(logits, table)
    B, V = kept.shape
    H = table.hist.shape[1]
    tokens = torch.zeros(B, dtype=torch.long, device=logits.device)
    for b in range(B):
        if int(table.active[b]) == 0:
            continue
        if float(table.temperature[b]) == 0.0:
            hit = kept[b]
        else:
            u = sample_uniform(int(table.seed[b]) & _M32, table.step[b].reshape(()), 0)
            hit = kept[b] & (cdf[b] > u)
        if bool(hit.any()):
            tok = int(hit.to(torch.uint8).argmax())
        else:  # the CDF's rounding at the upper edge; a row without a finite logit returns 0
            tok = int(kept[b].nonzero().max()) if bool(kept[b].any()) else 0
        tokens[b] = tok
        n = int(table.hist_len[b])
        if 0 <= n < H:
            table.hist[b, n] = tok
            table.hist_len[b] = n + 1
        table.step[b] += 1
        if info is not None:
            info[b, 0] = int(kept[b].sum())
            info[b, 1] = cut[b : b + 1].float().view(torch.int32)[0]
    return tokens


def sample_rows(logits: torch.Tensor, table: RowTable, want_info: Union[bool, torch.Tensor] = False):
    """One token per row of ``logits [B, V]``, each row with its own entry of ``table`` (:class:`RowTable`; a
    ``table.rows(r, r + 1)`` slice serves a ``[1, V]`` call).  Per active row: the tokens in ``hist[b, :hist_len[b]]``
    are penalised (``rep`` as in CTRL: a positive logit is multiplied by ``inv_rep``, any other by ``rep``; then
    ``presence`` is subtracted), top-k / top-p / temperature are :func:`sample_logits`'s over the penalised row with the
    row's own values, and the uniform is ``sample_uniform(seed[b], step[b], 0)`` -- a function of the request alone.
    ``temperature == 0`` is greedy: the lowest index among the maxima.  The same launch writes the token to
    ``hist[b, hist_len[b]]`` and advances ``hist_len[b]`` (a full history skips the append) and ``step[b]``.  An
    inactive row returns 0 and nothing of it is written.  Device operations only: graph-capturable.

    ``want_info``: also ``info [B, 2]`` int32 = (number of kept tokens, bits of the fp32 cut) -- for a greedy row the
    number of maxima and the maximum; a tensor is written in place (inactive rows keep their entries), ``True``
    allocates zeros.  ``V`` is at most ``ext().sample_rows_max_vocab()`` (2^20) on the GPU: the bitmap lives in LDS."""
    if logits.dim() != 2:
        raise ValueError(f"sample_rows: logits must be [B, V], got {tuple(logits.shape)}")
    if logits.dtype not in (torch.bfloat16, torch.float16, torch.float32):
        raise ValueError(f"sample_rows: logits must be bf16, fp16 or fp32, got {logits.dtype}")
    _check_table(logits, table)
    info = None
    if torch.is_tensor(want_info):
        info = want_info
        if info.dtype != torch.int32 or info.shape != (logits.shape[0], 2) or info.device != logits.device \
                or not info.is_contiguous():
            raise ValueError("sample_rows: info must be a contiguous int32 [B, 2] on the logits' device")
    elif want_info:
        info = torch.zeros(logits.shape[0], 2, dtype=torch.int32, device=logits.device)
    if use_native(logits):
        tokens = ext().sample_rows(logits, *table.columns, table.hist, info)
    else:
        tokens = _sample_rows_torch(logits, table, info)
    return tokens if info is None else (tokens, info)
