"""Token samplers over logits [b, s, V] (reference ``transformer/inference/sample.py``)."""
from __future__ import annotations

from typing import Optional

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
