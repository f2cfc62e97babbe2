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

Paged cache (``page_size=``, opt-in): the same static batch over a ``PagedKVCache`` -- one pool of pages per layer, a
block table per row, pages handed out by one host-side ``PageAllocator`` as the rows grow (``step`` gives a row a page
before the step that first writes into it).  ``ContinuousBatchDecoder`` builds continuous batching on it: a row whose
request has finished is released and refilled with the next request while the other rows go on, under one captured graph.
"""
from __future__ import annotations

from typing import Any, Callable, Optional, Sequence

import torch

from ...ops import gemm as gemm_ops
from ...core.nn.attention.attention import (BatchDecodeState, BatchStaticKVCache, BatchStaticKVCacheFP8, KVCache,
                                            PageAllocator, PagedDecodeState, PagedKVCache, PagedKVCacheFP8,
                                            ParallelSelfAttention, check_kv_cache_scheme, check_page_size)
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
    ``skinny_gemm``.

    ``page_size`` (opt-in, a multiple of 32): the cache is a ``PagedKVCache`` (``PagedKVCacheFP8``) of ``num_pages``
    pages (default: the parking pages plus ``ceil(capacity / page_size)`` pages per row) instead of one slab per row.
    A row gets ``ceil((n + 1) / page_size)`` pages for its prompt and one more whenever its write position starts a new
    page; ``step`` raises ``RuntimeError`` before it steps if the pool has none left.  Tokens and logits are those of
    the slab cache when both split plans coincide (``capacity`` a whole number of pages)."""

    def __init__(self, module: Any, prompt_lengths: Sequence[int], max_tokens: int, first_tokens: torch.Tensor,
                 sample_fn: Callable[[torch.Tensor], torch.Tensor], prefill_logits: torch.Tensor,
                 skinny_gemm: bool = False, kv_cache: Optional[str] = None, page_size: Optional[int] = None,
                 num_pages: Optional[int] = None) -> None:
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
        self.attns = [m for m in module.modules() if isinstance(m, ParallelSelfAttention)]
        assert self.attns, "no attention layers"
        self.page_size = None if page_size is None else check_page_size(page_size, "BatchDecoder")
        self.allocator: Optional[PageAllocator] = None
        self.pages: Optional[list[list[int]]] = None
        self._n_host = [int(n) for n in prompt_lengths]
        if self.page_size is None:
            self.state = BatchDecodeState(prompt_lengths, self.capacity, dev)
        else:
            page = self.page_size
            max_pages = -(-self.capacity // page)
            num_pages = B * (1 + max_pages) if num_pages is None else int(num_pages)
            self.allocator = PageAllocator(num_pages, reserved=B)
            self.pages = []
            for n in self._n_host:  # raises before anything is written
                self.pages.append(self.allocator.alloc(-(-(n + 1) // page)))
            self.state = PagedDecodeState(B, max_pages, page, num_pages, dev)
            for b, n in enumerate(self._n_host):
                self.state.assign(b, self.pages[b], n)
        if self.kv_cache is not None:
            for a in self.attns:
                a.check_fp8_kv_cache()
        for a in self.attns:
            kvs = [a.cache.get(b) for b in range(B)]
            assert all(isinstance(kv, KVCache) for kv in kvs), "batched decoding starts from B prefilled KV caches"
            assert [kv.length for kv in kvs] == list(prompt_lengths)
            for b in range(1, B):
                del a.cache[b]
            if self.page_size is None:
                cache_cls = BatchStaticKVCache if self.kv_cache is None else BatchStaticKVCacheFP8
                a.cache[0] = cache_cls.from_caches(kvs, self.state)
            else:
                paged_cls = PagedKVCache if self.kv_cache is None else PagedKVCacheFP8
                pool = paged_cls.empty(kvs[0].k.shape[1], kvs[0].k.shape[2], kvs[0].k.dtype, self.state)
                for b, kv in enumerate(kvs):
                    pool.load_row(b, kv, self.pages[b])
                a.cache[0] = pool
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
        if self.pages is not None:
            self._grow_pages()
        if self.graph is not None:
            self.graph.replay()
        else:
            with torch.no_grad():
                self._step()
        self.steps_done += 1

    def _grow_pages(self) -> None:
        """Paged cache: a page for every row whose write position (prompt length + steps since the prefill) starts a
        page it does not own yet.  All of them are taken at once, so an exhausted pool raises before anything changed."""
        assert self.pages is not None and self.allocator is not None and isinstance(self.state, PagedDecodeState)
        page = self.state.page
        need = [b for b, n in enumerate(self._n_host) if (n + self.steps_done - 1) // page >= len(self.pages[b])]
        if not need:
            return
        for b, pg in zip(need, self.allocator.alloc(len(need))):
            self.pages[b].append(pg)
            self.state.set_page(b, len(self.pages[b]) - 1, pg)

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


class _Request:
    """Host-side record of the request a decoder row holds."""

    def __init__(self, index: Any, n_prompt: int, max_tokens: int, pages: list[int]) -> None:
        self.index, self.n_prompt, self.max_tokens, self.pages = index, n_prompt, max_tokens, pages
        self.steps = 0  # decode steps since admit: the next step writes position n_prompt + steps
        self.tokens: list[int] = []
        self.logits: list[torch.Tensor] = []
        self.done = False


class ContinuousBatchDecoder:
    """Continuous batching over a paged KV cache: ``max_batch`` rows, one pool of pages per attention layer, one step
    (captured once as a HIP graph with ``use_cuda_graph``).  A row holds a request from ``admit`` to ``release``; the
    rows without one are parked (``PagedDecodeState``).  Admissions, releases and page allocations change device
    *values* (block table, positions, lengths, tokens) at fixed addresses, so the graph is never recaptured
    (``captures`` counts them).

    The step is ``BatchDecoder``'s: up to 4 rows on the GEMV kernels, 3..16 rows on the skinny MFMA kernels with
    ``skinny_gemm=True``; under the graph ``max_batch`` is limited to 4, or 16 with ``skinny_gemm``.  ``kv_cache`` is
    None or ``"fp8_e4m3"``.

    ``max_pages`` pages of ``page_size`` tokens bound one request (prompt + ``max_tokens``); ``num_pages`` sizes the pool
    (default: ``max_batch`` full-length requests plus the ``max_batch`` parking pages).  Every step records the sampled
    tokens and their logits of all rows into a ring of ``record_steps`` slots (``rec_tokens`` ``[R, B]``, ``rec_logits``
    ``[R, B, V]``); ``serve`` reads it back once per ``check_every <= record_steps`` steps and files the rows' entries
    under their requests.

    Not here: preemption or swapping when the pool is full (``admit`` / ``step`` raise), prefix sharing, paged or
    batched prefill (a prompt is prefilled alone by the existing eager path and copied into its pages)."""

    def __init__(self, module: Any, max_batch: int, page_size: int = 64, max_pages: int = 1,
                 num_pages: Optional[int] = None, sample_fn: Optional[Callable[[torch.Tensor], torch.Tensor]] = None,
                 skinny_gemm: bool = False, kv_cache: Optional[str] = None, use_cuda_graph: bool = False,
                 record_steps: int = 8) -> None:
        from .sample import sample_argmax

        self.module = module
        self.skinny_gemm = bool(skinny_gemm)
        self.kv_cache = check_kv_cache_scheme(kv_cache, "ContinuousBatchDecoder")
        page = check_page_size(page_size, "ContinuousBatchDecoder")
        B = int(max_batch)
        if B < 1 or max_pages < 1 or record_steps < 1:
            raise ValueError("ContinuousBatchDecoder: max_batch, max_pages and record_steps must be at least 1")
        limit = gemm_ops.SKINNY_MAX_ROWS if skinny_gemm else gemm_ops.GEMV_MAX_ROWS
        if use_cuda_graph and B > limit:
            raise ValueError(
                f"ContinuousBatchDecoder: use_cuda_graph{' with skinny_gemm' if skinny_gemm else ''} supports at most "
                f"{limit} rows, got {B}: above that the linear layers run library GEMMs, whose algorithm choice under "
                "graph capture need not be the eager one; run without use_cuda_graph")
        self.attns = [m for m in module.modules() if isinstance(m, ParallelSelfAttention)]
        assert self.attns, "no attention layers"
        if self.kv_cache is not None:
            for a in self.attns:
                a.check_fp8_kv_cache()
        p0 = next(self.attns[0].parameters())
        dev = p0.device
        self.batch_size, self.page_size, self.max_pages = B, page, int(max_pages)
        num_pages = B * (1 + self.max_pages) if num_pages is None else int(num_pages)
        self.allocator = PageAllocator(num_pages, reserved=B)
        self.state = PagedDecodeState(B, self.max_pages, page, num_pages, dev)
        # the model's own bound on a sequence: the rotary table's rows (None: no such table)
        tables = [a.rotary_embedding.cos_table.shape[0] for a in self.attns
                  if getattr(a.rotary_embedding, "cos_table", None) is not None]
        self.sequence_limit: Optional[int] = min(tables) if tables else None
        paged_cls = PagedKVCache if self.kv_cache is None else PagedKVCacheFP8
        for a in self.attns:
            a.cache.clear()
            a.cache[0] = paged_cls.empty(a.num_kv_heads_per_partition, a.hidden_size_per_attention_head, p0.dtype,
                                         self.state)
        self.spare_index = 1  # the cache index a prompt is prefilled under before it is copied into its pages
        self.rows: list[Optional[_Request]] = [None] * B
        self.tok = torch.zeros(B, 1, dtype=torch.long, device=dev)
        settings = InferenceSettings(use_cache=True, reset_cache=False, cache_index=0, embedding_layers=[-1])
        cu_q = torch.arange(B + 1, dtype=torch.int32, device=dev)
        self.batch = TextDatasetBatch(input_token_ids=self.tok, position_ids=self.state.pos.view(B, 1),
                                      cumulative_seq_lengths=cu_q, cumulative_seq_lengths_padded=cu_q,
                                      inference_settings=settings)
        self.sample_fn = sample_fn if sample_fn is not None else sample_argmax
        self.record_steps = int(record_steps)
        self._slot = torch.zeros(1, dtype=torch.long, device=dev)
        # one parked step sizes the recording ring (vocabulary, logits dtype) and warms the lazy module state
        with torch.no_grad(), gemm_ops.skinny_gemm(self.skinny_gemm):
            act = self.module.forward(self.batch).activations
        self.rec_tokens = torch.zeros(self.record_steps, B, dtype=torch.long, device=dev)
        self.rec_logits = torch.zeros(self.record_steps, B, act.shape[-1], dtype=act.dtype, device=dev)
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self.captures = 0
        self.steps_run = 0
        if use_cuda_graph:
            self.capture()
        self._settle()

    # ------------------------------------------------------------------ the step
    def _step(self) -> None:
        """One decode step of all rows, device ops only: feed ``tok`` at ``pos``, sample into ``tok``, record into the
        ring slot, advance the live rows."""
        B = self.batch_size
        with gemm_ops.skinny_gemm(self.skinny_gemm):
            out = self.module.forward(self.batch)
        act = out.activations
        nxt = self.sample_fn(act).reshape(B, 1)
        self.tok.copy_(nxt)
        self.rec_tokens.index_copy_(0, self._slot, nxt.reshape(1, B))
        self.rec_logits.index_copy_(0, self._slot, act[:, -1, :].unsqueeze(0))
        self._slot.add_(1).remainder_(self.record_steps)
        self.state.advance()

    def _settle(self) -> None:
        """After the parked warm-up / capture passes: tokens, ring slot, error word and sampler counter as new."""
        self.tok.zero_()
        self._slot.zero_()
        self.state.err.zero_()
        if hasattr(self.sample_fn, "reset"):
            self.sample_fn.reset(0)

    def capture(self) -> None:
        """Captures the step, once, while every row is parked (the passes write parking pages only)."""
        assert self.tok.is_cuda, "graph-captured decoding needs a GPU"
        assert all(r is None for r in self.rows), "capture before the first admit"
        side = torch.cuda.Stream(device=self.tok.device)
        side.wait_stream(torch.cuda.current_stream(self.tok.device))
        with torch.cuda.stream(side), torch.no_grad():
            self._step()
        torch.cuda.current_stream(self.tok.device).wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(g):
            self._step()
        self.graph = g
        self.captures += 1
        self._settle()

    # ------------------------------------------------------------------ rows
    @property
    def free_rows(self) -> list[int]:
        return [b for b, r in enumerate(self.rows) if r is None]

    def admit(self, row: int, input_tokens: Sequence[int], max_tokens: int, index: Any = None) -> _Request:
        """Row ``row`` takes a request: the prompt is prefilled (eager, alone), its K/V copied into freshly allocated
        pages, the row's device state set and its first token drawn with one ``sample_fn`` call on the prefill logits.
        ``ValueError`` for a request that cannot fit ``max_pages`` pages or the model's sequence length, ``RuntimeError``
        naming the pool size when the pool lacks the prompt's pages -- both before anything is written."""
        n = len(input_tokens)
        if n < 1 or max_tokens < 1:
            raise ValueError("ContinuousBatchDecoder.admit: empty prompt or max_tokens < 1")
        if n + max_tokens > self.state.capacity:
            raise ValueError(f"ContinuousBatchDecoder.admit: prompt ({n}) + max_tokens ({max_tokens}) exceeds max_pages * "
                             f"page_size = {self.max_pages} * {self.page_size} = {self.state.capacity}")
        if self.sequence_limit is not None and n + max_tokens > self.sequence_limit:
            raise ValueError(f"ContinuousBatchDecoder.admit: prompt ({n}) + max_tokens ({max_tokens}) exceeds the model's "
                             f"sequence length {self.sequence_limit}")
        if self.rows[row] is not None:
            raise ValueError(f"ContinuousBatchDecoder.admit: row {row} holds a request (release it first)")
        pages = self.allocator.alloc(-(-(n + 1) // self.page_size))  # RuntimeError before anything is written
        settings = InferenceSettings(use_cache=True, reset_cache=True, cache_index=self.spare_index, embedding_layers=[-1])
        with torch.no_grad():
            try:
                out = self.module.forward(TextDatasetBatch(input_token_ids=torch.tensor(list(input_tokens)).unsqueeze(0),
                                                           inference_settings=settings))
            except BaseException:
                self.allocator.free(pages)
                raise
            for a in self.attns:
                kv = a.cache.pop(self.spare_index)
                assert isinstance(kv, KVCache) and kv.length == n
                a.cache[0].load_row(row, kv, pages)
            last = out.activations[:, -1:, :]
            first = self.sample_fn(last).reshape(1, 1).to(torch.long)
            self.state.assign(row, pages, n)
            self.tok[row : row + 1].copy_(first)
        req = _Request(index, n, int(max_tokens), pages)
        req.tokens.append(int(first.item()))
        req.logits.append(last.reshape(1, -1))
        self.rows[row] = req
        return req

    def release(self, row: int) -> Optional[_Request]:
        """The row's pages go back to the free list and the row is parked; returns the request it held."""
        req = self.rows[row]
        if req is None:
            return None
        self.allocator.free(req.pages)
        self.state.park(row)
        self.tok[row : row + 1].zero_()
        self.rows[row] = None
        return req

    def step(self) -> None:
        """One step of all rows.  First every live row whose write position starts a page it does not own gets one (all
        taken at once: an exhausted pool raises ``RuntimeError`` naming the pool size before anything is stepped) and
        the new table entries are copied to the device; then the graph is replayed, or the step run eagerly."""
        live = [(b, r) for b, r in enumerate(self.rows) if r is not None]
        need = []
        for b, r in live:
            p = r.n_prompt + r.steps
            if p >= self.state.capacity:
                raise RuntimeError(f"ContinuousBatchDecoder.step: row {b} is at position {p}, past its {self.max_pages} "
                                   f"pages of {self.page_size}")
            if p // self.page_size >= len(r.pages):
                need.append((b, r))
        if need:
            for (b, r), pg in zip(need, self.allocator.alloc(len(need))):
                r.pages.append(pg)
                self.state.set_page(b, len(r.pages) - 1, pg)
        if self.graph is not None:
            self.graph.replay()
        else:
            with torch.no_grad():
                self._step()
        for _, r in live:
            r.steps += 1
        self.steps_run += 1

    # ------------------------------------------------------------------ the serving loop
    def serve(self, requests: Sequence[tuple[Sequence[int], int]], stop_tokens: Sequence[int],
              check_every: int = 8) -> list[tuple[list[int], torch.Tensor]]:
        """Runs ``requests`` = [(prompt tokens, max_tokens), ...] to completion, in arrival order: free rows are filled,
        all rows step, and every ``check_every`` steps (fewer when a row would pass its ``max_tokens``) the recorded
        tokens are read back; a request is cut at its first stop token or its ``max_tokens``, its row released and
        refilled.  Returns (tokens, logits ``[len(tokens), V]``) per request, in request order."""
        stops = set(int(t) for t in stop_tokens)
        check_every = max(1, min(int(check_every), self.record_steps))
        results: list[Optional[tuple[list[int], torch.Tensor]]] = [None] * len(requests)
        nxt = 0

        def finish(row: int) -> None:
            req = self.release(row)
            assert req is not None
            results[req.index] = (req.tokens, torch.cat(req.logits))

        def over(req: _Request) -> bool:
            return req.tokens[-1] in stops or len(req.tokens) >= req.max_tokens

        while nxt < len(requests) or any(r is not None for r in self.rows):
            for row in self.free_rows:
                while nxt < len(requests) and self.rows[row] is None:
                    toks, mt = requests[nxt]
                    req = self.admit(row, toks, mt, index=nxt)
                    nxt += 1
                    if over(req):  # done with the prefill's token
                        finish(row)
            live = [(b, r) for b, r in enumerate(self.rows) if r is not None]
            if not live:
                continue
            k = min(check_every, min(r.max_tokens - len(r.tokens) for _, r in live))
            self._slot.zero_()
            for _ in range(k):
                self.step()
            self.state.check()
            got = self.rec_tokens[:k].tolist()
            logits = self.rec_logits[:k].clone()
            for b, r in live:
                for i in range(k):
                    r.tokens.append(got[i][b])
                    if over(r):
                        k_row = i + 1
                        break
                else:
                    k_row = k
                r.logits.append(logits[:k_row, b])
                if over(r):
                    finish(b)
        return [r for r in results if r is not None]
