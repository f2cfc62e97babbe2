"""Token samplers over logits [b, s, V] (reference ``transformer/inference/sample.py``)."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence, Union

import torch
import torch.nn.functional as F


def sample_argmax(logits: torch.Tensor) -> torch.Tensor:
    return torch.argmax(logits, dim=-1)[:, -1]


def fast_multinomial(p: torch.Tensor) -> torch.Tensor:
    """One draw per row of ``p`` (inverse CDF; cheaper than torch.multinomial for a single sample)."""
    u = torch.rand(p.shape[:-1], device=p.device)[..., None]
    return (p.cumsum(-1) >= u).byte().argmax(-1)


def sample_temperature(logits: torch.Tensor, temperature: float = 1.0) -> torch.Tensor:
    return fast_multinomial(F.softmax(logits / temperature, dim=-1))[:, -1]


def top_k_transform(logits: torch.Tensor, k: int = 10) -> torch.Tensor:
    kth = torch.topk(logits, k)[0][..., -1, None]
    return logits.masked_fill(logits < kth, float("-inf"))


def top_p_transform(logits: torch.Tensor, threshold: float = 0.95) -> torch.Tensor:
    """Nucleus filtering of a 1-D logits vector: keep the smallest prefix of sorted tokens whose
    probability mass exceeds ``threshold`` (the first token is always kept)."""
    sorted_logits, order = torch.sort(logits, descending=True, dim=-1)
    cum = torch.cumsum(F.softmax(sorted_logits, dim=-1), dim=-1)
    drop = cum > threshold
    drop[1:] = drop[:-1].clone()
    drop[0] = False
    out = logits.clone()
    out[order[drop]] = float("-inf")
    return out


class Sampler:
    """Seeded top-k / top-p / temperature sampler that graph-captured decoding can use: one fused launch
    (``ops.sample.sample_logits``), device operations only.  Callable on ``logits [b, s, V]`` like the functions above
    (last position, returns ``[b]``).  The draw of call ``n`` is a hash of ``(seed, n, row)``; ``n`` lives in a device
    int64 counter (created on the logits' device at the first call) that every call advances on the device, so a
    graph replay draws the number the eager loop would.  ``reset(step)`` sets the counter."""

    graph_safe = True

    def __init__(self, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0) -> None:
        if not temperature > 0:
            raise ValueError("Sampler: temperature must be positive (top_k=1 is greedy)")
        self.temperature = float(temperature)
        self.top_k = int(top_k)
        self.top_p = float(top_p)
        self.seed = int(seed)
        self._step: Optional[torch.Tensor] = None
        self._start = 0

    def reset(self, step: int = 0) -> None:
        self._start = int(step)
        if self._step is not None:
            self._step.fill_(self._start)

    @property
    def step(self) -> int:
        """The counter's value (reads the device)."""
        return self._start if self._step is None else int(self._step.item())

    def __call__(self, logits: torch.Tensor) -> torch.Tensor:
        from ...ops.sample import sample_logits

        if self._step is None or self._step.device != logits.device:
            self._step = torch.full((1,), self.step, dtype=torch.long, device=logits.device)
        tokens = sample_logits(logits[:, -1, :], self._step, self.seed, self.temperature, self.top_k, self.top_p)
        self._step.add_(1)
        return tokens


@dataclass(frozen=True)
class SamplingParams:
    """One request's sampling: ``temperature`` 0 is greedy; ``top_k`` / ``top_p`` as in ``Sampler``; ``seed`` is the
    request's own; ``repetition_penalty`` r divides the positive and multiplies the other logits of the tokens the
    request has seen, ``presence_penalty`` is subtracted from them (1 and 0: off); ``penalize_prompt``: the prompt
    counts as seen, not only what the request has drawn."""

    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    seed: int = 0
    repetition_penalty: float = 1.0
    presence_penalty: float = 0.0
    penalize_prompt: bool = True

    def check(self) -> "SamplingParams":
        if not (self.temperature >= 0 and math.isfinite(self.temperature)):
            raise ValueError("SamplingParams: temperature must be finite and not negative (0 is greedy)")
        if not math.isfinite(self.top_p):
            raise ValueError("SamplingParams: top_p must be finite")
        if not (self.repetition_penalty > 0 and math.isfinite(self.repetition_penalty)):
            raise ValueError("SamplingParams: repetition_penalty must be finite and positive")
        if not math.isfinite(self.presence_penalty):
            raise ValueError("SamplingParams: presence_penalty must be finite")
        return self


def per_request(sampling: Union[SamplingParams, Sequence[SamplingParams]], n: int, where: str) -> list[SamplingParams]:
    """``sampling`` as ``n`` checked ``SamplingParams``: one for all, or a list / tuple of ``n``; anything else is a
    ``ValueError``."""
    given = list(sampling) if isinstance(sampling, (list, tuple)) else [sampling] * n
    if len(given) != n or not all(isinstance(p, SamplingParams) for p in given):
        raise ValueError(f"{where}: sampling must be one SamplingParams or one per request ({n})")
    return [p.check() for p in given]


class RequestSampler:
    """Per-request sampling for continuous batching: every decoder row has its own ``SamplingParams``, its own draw
    counter and its own token history in a device-resident ``ops.sample.RowTable`` of ``max_batch`` rows and
    ``history`` tokens per row, and a step is one fused launch (``ops.sample.sample_rows``) that draws, appends the
    token to the row's history and advances its counter.  A draw is a hash of the request's ``(seed, draw number)``:
    what a request samples depends neither on its row, nor on its neighbours, nor on when it was admitted.

    ``set_row`` fills a row (one copy from pinned memory, asynchronous on a GPU), ``first`` draws a just admitted
    request's first token on the one-row slice of the table, ``__call__`` is the step's draw on ``[B, 1, V]`` logits,
    ``clear_row`` parks a row: a parked row returns token 0 and changes nothing, so a decoder's warm-up and capture
    passes over parked rows burn no draws and ``reset`` has nothing to rewind."""

    graph_safe = True

    def __init__(self, max_batch: int, history: int, device: Union[None, str, int, torch.device] = None) -> None:
        from ...ops.sample import RowTable

        self.max_batch, self.history = int(max_batch), int(history)
        self.table = RowTable.empty(self.max_batch, self.history, device)
        buf = self.table.buf
        # one staging row per table row: a row's copy may still be in flight when the next row is filled
        self._stage = torch.zeros(buf.shape, dtype=buf.dtype, pin_memory=buf.is_cuda)
        self._stage_f = self._stage.view(torch.float32)

    def reset(self, step: int = 0) -> None:
        """Nothing to rewind: the counters belong to the requests."""

    def set_row(self, row: int, params: SamplingParams, prompt_tokens: Sequence[int] = ()) -> None:
        """Row ``row`` takes a request: its parameters, draw counter 0 and history = the prompt (empty without
        ``penalize_prompt``).  ``ValueError`` for bad parameters or a prompt longer than ``history``, before anything
        is written."""
        from ...ops.sample import _HEADER, _OFFSETS, _seed32

        params.check()
        if not 0 <= row < self.max_batch:
            raise ValueError(f"RequestSampler: row {row} outside 0..{self.max_batch - 1}")
        hist = list(prompt_tokens) if params.penalize_prompt else []
        if len(hist) > self.history:
            raise ValueError(f"RequestSampler: a prompt of {len(hist)} tokens exceeds the history of {self.history}")
        seed = _seed32(params.seed)
        rep = float(torch.tensor(params.repetition_penalty, dtype=torch.float32))
        ints = {"active": 1, "top_k": max(-1, min(int(params.top_k), 2**31 - 1)), "seed": seed - (seed >> 31 << 32),
                "hist_len": len(hist)}
        floats = {"temperature": params.temperature, "top_p": params.top_p, "rep": rep, "inv_rep": 1.0 / rep,
                  "presence": params.presence_penalty}
        s, sf = self._stage[row], self._stage_f[row]
        s[_OFFSETS["step"] : _OFFSETS["step"] + 2] = 0
        for name, value in ints.items():
            s[_OFFSETS[name]] = value
        for name, value in floats.items():
            sf[_OFFSETS[name]] = value
        if hist:
            s[_HEADER : _HEADER + len(hist)] = torch.tensor(hist, dtype=torch.int32)
        n = _HEADER + len(hist)
        self.table.buf[row, :n].copy_(s[:n], non_blocking=True)

    def clear_row(self, row: int) -> None:
        self.table.active[row : row + 1].zero_()

    def clear(self) -> None:
        self.table.active.zero_()

    def first(self, row: int, logits: torch.Tensor) -> torch.Tensor:
        """The first token of the request in ``row`` from its prefill ``logits [1, s, V]`` (last position)."""
        from ...ops.sample import sample_rows

        return sample_rows(logits[:, -1, :], self.table.rows(row, row + 1))

    def __call__(self, logits: torch.Tensor) -> torch.Tensor:
        from ...ops.sample import sample_rows

        if logits.shape[0] != self.max_batch:
            raise ValueError(f"RequestSampler: {logits.shape[0]} rows of logits for a table of {self.max_batch}")
        return sample_rows(logits[:, -1, :], self.table)
