"""Batched token-by-token generation: B prompts of different lengths share every decode step, so the weights
stream once per step for B tokens (``graph_decode.GraphDecoder`` is the one-sequence form).

* The prompts are prefilled one at a time by the existing code, prompt b under ``cache_index = b``.
* Every attention layer's B ``KVCache``s become ONE ``BatchStaticKVCache`` ``[B * cap, nkv, hd]`` (``cap`` = longest
  prompt + ``max_tokens``) under ``cache_index = 0``, sharing one ``BatchDecodeState``: a position per row and the
  ``(start, length)`` key range the flash-decoding kernel reads for it.  Addresses and shapes are the same at every
  step and for every mix of lengths, so the step can be captured as ONE HIP graph.
* A step forwards the ``[B, 1]`` token buffer (one query segment per row, ``position_ids`` = the state's ``pos``),
  samples, records tokens and logits at the device-side step index and advances the positions.  The same ``_step``
  is the eager loop and the captured graph: both run the same kernels.

Up to ``ops.gemm.GEMV_MAX_ROWS`` (4) rows a step runs the weight-streaming GEMV kernels (bf16 or FP8 copies) with
their fused norm / SwiGLU / residual epilogues plus one batched RoPE + K/V append launch per layer; above that the
library GEMMs and the unfused norm / SwiGLU kernels.  Graph capture is limited to 4 rows: above them
``ops.gemm.linear`` uses a cached hipBLASLt plan in eager mode but torch's own path under capture, and the two need
not pick the same algorithm, so graph tokens could differ from eager tokens.

``skinny_gemm=True`` (opt-in) runs every step -- eager, warm-up and capture alike -- inside
``ops.gemm.skinny_gemm()``: ``ops.gemm.SKINNY_MIN_ROWS`` to 16 rows then take the MFMA weight-streaming kernels
(``csrc/kernels/skinny.hip``, bf16 / fp16 or FP8 copies, the same fused epilogues), whose time does not grow with the
row count and whose rows do not depend on each other, and the graph limit becomes 16 rows.  Above 16 rows the eager
loop runs the library path as without the flag.

Sampling: the first token of all rows is ONE ``sample_fn`` call on the stacked ``[B, 1, V]`` prefill logits (step 0,
rows 0..B-1) and every later step is one call on the step's ``[B, 1, V]`` logits.  ``sample.Sampler`` hashes
``(seed, step, row)``, and the row index is part of the draw: a sampled batch does NOT repeat the text each prompt
would get alone (where it is always row 0).  Greedy decoding (``sample_argmax``) does not depend on the row.
"""
from __future__ import annotations

from typing import Any, Callable, Optional, Sequence

import torch

from ...ops import gemm as gemm_ops
from ...core.nn.attention.attention import (BatchDecodeState, BatchStaticKVCache, BatchStaticKVCacheFP8, KVCache,
                                            ParallelSelfAttention, check_kv_cache_scheme)
from ..data import TextDatasetBatch
from ..data.inference_settings import InferenceSettings


class BatchDecoder:
    """Decode loop over B prefilled prompts (attention caches ``0 .. B-1`` hold their ``KVCache``s).

    ``tok`` ``[B, 1]`` int64 is the static token buffer a step feeds and then overwrites with the tokens it sampled.
    A caller may overwrite it between steps (teacher forcing, a serving loop that substitutes tokens).
    ``tokens`` ``[max_tokens, B]`` and ``logits`` ``[max_tokens, B, V]`` record every step; row 0 of both is the
    prefill's.

    ``kv_cache="fp8_e4m3"`` (opt-in): the batched cache holds e4m3 codes with one power-of-two scale per cached row
    (``BatchStaticKVCacheFP8``: the prefilled rows are quantised here, every step appends quantised rows and the
    flash-decoding kernel reads the codes).  It touches attention only, so it composes with FP8 weights and
    ``skinny_gemm``."""

    def __init__(self, module: Any, prompt_lengths: Sequence[int], max_tokens: int, first_tokens: torch.Tensor,
                 sample_fn: Callable[[torch.Tensor], torch.Tensor], prefill_logits: torch.Tensor,
                 skinny_gemm: bool = False, kv_cache: Optional[str] = None) -> None:
        self.module = module
        self.skinny_gemm = bool(skinny_gemm)
        self.kv_cache = check_kv_cache_scheme(kv_cache, "BatchDecoder")
        dev = first_tokens.device
        B = len(prompt_lengths)
        assert B >= 1 and max_tokens >= 1 and first_tokens.numel() == B and prefill_logits.shape[0] == B
        self.batch_size = B
        self.max_tokens = max_tokens
        self.capacity = max(prompt_lengths) + max_tokens
        self.n_prompt = torch.tensor(list(prompt_lengths), dtype=torch.long, device=dev)
        self.state = BatchDecodeState(prompt_lengths, self.capacity, dev)
        self.attns = [m for m in module.modules() if isinstance(m, ParallelSelfAttention)]
        assert self.attns, "no attention layers"
        cache_cls = BatchStaticKVCache if self.kv_cache is None else BatchStaticKVCacheFP8
        if self.kv_cache is not None:
            for a in self.attns:
                a.check_fp8_kv_cache()
        for a in self.attns:
            kvs = [a.cache.get(b) for b in range(B)]
            assert all(isinstance(kv, KVCache) for kv in kvs), "batched decoding starts from B prefilled KV caches"
            assert [kv.length for kv in kvs] == list(prompt_lengths)
            for b in range(1, B):
                del a.cache[b]
            a.cache[0] = cache_cls.from_caches(kvs, self.state)
        V = prefill_logits.shape[-1]
        rows = max(max_tokens, 2)  # the warm-up / capture passes record a step 1 even when max_tokens is 1
        self.first = first_tokens.reshape(B, 1).to(torch.long).clone()
        self.tok = self.first.clone()
        self.tokens = torch.zeros(rows, B, dtype=torch.long, device=dev)
        self.logits = torch.zeros(rows, B, V, dtype=prefill_logits.dtype, device=dev)
        self.tokens[0].copy_(self.first.view(B))
        self.logits[0].copy_(prefill_logits.reshape(B, V))
        settings = InferenceSettings(use_cache=True, reset_cache=False, cache_index=0, embedding_layers=[-1])
        cu_q = torch.arange(B + 1, dtype=torch.int32, device=dev)
        self.batch = TextDatasetBatch(input_token_ids=self.tok, position_ids=self.state.pos.view(B, 1),
                                      cumulative_seq_lengths=cu_q, cumulative_seq_lengths_padded=cu_q,
                                      inference_settings=settings)
        self.sample_fn = sample_fn
        self._step_idx = torch.ones(1, dtype=torch.long, device=dev)  # the step being computed (0 is the prefill's)
        self.steps_done = 1
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self._rewind()

    def _step(self) -> None:
        """One decode step, device ops only: feed ``tok`` at ``pos``, sample into ``tok``, record, advance."""
        B = self.batch_size
        with gemm_ops.skinny_gemm(self.skinny_gemm):
            out = self.module.forward(self.batch)
        act = out.activations
        nxt = self.sample_fn(act).reshape(B, 1)
        self.tok.copy_(nxt)
        self.tokens.index_copy_(0, self._step_idx, nxt.reshape(1, B))
        self.logits.index_copy_(0, self._step_idx, act[:, -1, :].unsqueeze(0))
        self._step_idx.add_(1)
        self.state.advance()

    def capture(self) -> None:
        assert self.tok.is_cuda, "graph-captured decoding needs a GPU"
        side = torch.cuda.Stream(device=self.tok.device)
        side.wait_stream(torch.cuda.current_stream(self.tok.device))
        with torch.cuda.stream(side), torch.no_grad():
            self._step()  # warm-up: allocator, library handles, lazy module state
        torch.cuda.current_stream(self.tok.device).wait_stream(side)
        self._rewind()
        g = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(g):
            self._step()
        self._rewind()  # capture records the work; it also ran it once (the state is reset before replay)
        self.graph = g

    def _rewind(self) -> None:
        self.state.reset(self.n_prompt)
        self.tok.copy_(self.first)
        self._step_idx.fill_(1)
        self.steps_done = 1
        if hasattr(self.sample_fn, "reset"):
            self.sample_fn.reset(1)  # step 0 drew the prefills' tokens; the warm-up and capture passes burn no draws

    def step(self) -> None:
        """Runs one step (a replay of the captured graph, or the eager step) on the current ``tok``."""
        assert self.steps_done < self.max_tokens, "all max_tokens steps are done"
        if self.graph is not None:
            self.graph.replay()
        else:
            with torch.no_grad():
                self._step()
        self.steps_done += 1

    def run(self, stop_tokens: Sequence[int], check_every: int = 8) -> list[tuple[list[int], torch.Tensor]]:
        """Runs the remaining steps until every row has produced a stop token or ``max_tokens`` is reached (the rows
        that have stopped keep stepping: the batch is static); per row, (tokens through its first stop token, their
        logits).  The tokens are read back every ``check_every`` steps."""
        stops = set(int(t) for t in stop_tokens)
        B = self.batch_size
        while True:
            got = self.tokens[: self.steps_done].tolist()  # [steps][B]
            cut = [next((i + 1 for i, row in enumerate(got) if row[b] in stops), None) for b in range(B)]
            if self.steps_done >= self.max_tokens or all(c is not None for c in cut):
                break
            for _ in range(min(check_every, self.max_tokens - self.steps_done)):
                self.step()
            self.state.check()
        out = []
        for b in range(B):
            n = cut[b] if cut[b] is not None else self.steps_done
            out.append(([row[b] for row in got[:n]], self.logits[:n, b]))
        return out
