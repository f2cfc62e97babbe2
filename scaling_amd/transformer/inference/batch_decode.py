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

``wide_batch=True`` (opt-in, implies the skinny path for 3..16 rows) runs every step inside
``ops.gemm.skinny_gemm(wide=True)``: 17 to ``ops.gemm.WIDE_MAX_ROWS`` (64) rows take the wide MFMA kernels
(``csrc/kernels/wide.hip``: x staged through LDS once per workgroup, every weight fragment feeding up to four MFMAs; the
same forms, quantised copies and fused epilogues, rows bitwise independent of each other) and the graph limit becomes
64 rows.  A request's tokens may differ between a B <= 16 and a B > 16 run: different kernels with different summation
orders serve them (as already between the GEMV and the skinny kernel).

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

import contextlib
from typing import Any, Callable, Optional, Sequence, Union

import torch

from ...ops import gemm as gemm_ops
from ...core.nn.attention.attention import (BatchDecodeState, BatchStaticKVCache, BatchStaticKVCacheFP8, ChunkPass,
                                            KVCache, PageAllocator, PagedDecodeState, PagedKVCache, PagedKVCacheFP8,
                                            ParallelSelfAttention, check_kv_cache_scheme, check_page_size)
from ..data import TextDatasetBatch
from ..data.inference_settings import InferenceSettings
from .sample import SamplingParams

SamplingArg = Union[None, SamplingParams, Sequence[SamplingParams]]  # None, one for all, or one per request


class BatchDecoder:
    """Decode loop over B prefilled prompts (attention caches ``0 .. B-1`` hold their ``KVCache``s).

    ``tok`` ``[B, 1]`` int64 is the static token buffer a step feeds and then overwrites with the tokens it sampled.
    A caller may overwrite it between steps (teacher forcing, a serving loop that substitutes tokens).
    ``tokens`` ``[max_tokens, B]`` and ``logits`` ``[max_tokens, B, V]`` record every step; row 0 of both is the
    prefill's.

    ``kv_cache="fp8_e4m3"`` (opt-in): the batched cache holds e4m3 codes with one power-of-two scale per cached row
    (``BatchStaticKVCacheFP8``: the prefilled rows are quantised here, every step appends quantised rows and the
    flash-decoding kernel reads the codes).  It touches attention only, so it composes with FP8 weights and
    ``skinny_gemm`` and ``wide_batch`` (the module docstring: 17..64 rows on the wide MFMA kernels).

    ``page_size`` (opt-in, a multiple of 32): the cache is a ``PagedKVCache`` (``PagedKVCacheFP8``) of ``num_pages``
    pages (default: the parking pages plus ``ceil(capacity / page_size)`` pages per row) instead of one slab per row.
    A row gets ``ceil((n + 1) / page_size)`` pages for its prompt and one more whenever its write position starts a new
    page; ``step`` raises ``RuntimeError`` before it steps if the pool has none left.  Tokens and logits are those of
    the slab cache when both split plans coincide (``capacity`` a whole number of pages)."""

    def __init__(self, module: Any, prompt_lengths: Sequence[int], max_tokens: int, first_tokens: torch.Tensor,
                 sample_fn: Callable[[torch.Tensor], torch.Tensor], prefill_logits: torch.Tensor,
                 skinny_gemm: bool = False, kv_cache: Optional[str] = None, page_size: Optional[int] = None,
                 num_pages: Optional[int] = None, wide_batch: bool = False) -> None:
        self.module = module
        self.wide_batch = bool(wide_batch)
        self.skinny_gemm = bool(skinny_gemm) or self.wide_batch
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
        with gemm_ops.skinny_gemm(self.skinny_gemm, wide=self.wide_batch):
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
    ``skinny_gemm=True``, 17..64 rows on the wide MFMA kernels with ``wide_batch=True`` (which implies ``skinny_gemm``);
    under the graph ``max_batch`` is limited to 4, 16 with ``skinny_gemm`` or 64 with ``wide_batch``.  ``kv_cache`` is
    None or ``"fp8_e4m3"``.

    ``max_pages`` pages of ``page_size`` tokens bound one request (prompt + ``max_tokens``); ``num_pages`` sizes the pool
    (default: ``max_batch`` full-length requests plus the ``max_batch`` parking pages).  Every step records the sampled
    tokens and their logits of all rows into a ring of ``record_steps`` slots (``rec_tokens`` ``[R, B]``, ``rec_logits``
    ``[R, B, V]``); ``serve`` reads it back once per ``check_every <= record_steps`` steps and files the rows' entries
    under their requests.

    ``prefill_chunk=C`` (opt-in, a positive multiple of 32; bf16 / fp16 models on one device, flash attention, no
    ``key_query_norm``): ``admit`` forwards the prompt in chunks of at most ``C`` tokens straight into its freshly
    allocated pages -- every layer rotates the chunk and writes its K/V rows with one launch
    (``ext().rope_kv_write_chunk``; ``PagedKVCache.write_rows`` on the CPU) and attends over the pool with
    ``ops.attention.chunk_attention`` (``csrc/kernels/flash_chunk.hip``) --, so no contiguous copy of the prompt's
    K/V, no spare cache index and no ``load_row``; activations are those of one chunk.  The captured step is not
    touched (``captures`` stays 1).  With ``kv_cache="fp8_e4m3"`` the later chunks read the earlier chunks' keys as e4m3
    codes: the prompt's own prefill then sees quantised K/V, which the unchunked admit (prefill against exact bf16
    K/V, quantised afterwards) does not.  Chunks at or below ``ops.gemm.decode_rows_limit()`` rows may run their
    linear layers on the decode kernels.  ``None`` (default) is the unchunked path, unchanged.

    ``admit_many`` admits several requests together (chunk j of every prompt as one packed pass); ``serve`` uses it
    whenever more than one row is free and more than one request waits.

    Per-request sampling (``sample_fn=sample.RequestSampler(max_batch, history >= max_pages * page_size)``, or
    ``sampling=True`` / a default ``SamplingParams`` to have one built): ``admit`` / ``admit_many`` / ``serve`` take
    ``sampling=`` (``SamplingParams``), the row's entry of the sampler's table is filled before the first token is drawn
    on the one-row slice, ``release`` parks it, and the captured step's single sampling launch serves every row with
    its own parameters, penalties, history and draw counter.  ``sampling=`` beside an ordinary ``sample_fn`` raises
    ``ValueError``.

    Not here: preemption or swapping when the pool is full (``admit`` / ``step`` raise), prefix sharing, batched
    prefill without ``prefill_chunk`` (a prompt is then prefilled alone), prefill chunks interleaved with decode steps
    inside the captured step."""

    def __init__(self, module: Any, max_batch: int, page_size: int = 64, max_pages: int = 1,
                 num_pages: Optional[int] = None, sample_fn: Optional[Callable[[torch.Tensor], torch.Tensor]] = None,
                 skinny_gemm: bool = False, kv_cache: Optional[str] = None, use_cuda_graph: bool = False,
                 record_steps: int = 8, wide_batch: bool = False, prefill_chunk: Optional[int] = None,
                 sampling: Union[None, bool, SamplingParams] = None) -> None:
        from .sample import RequestSampler, sample_argmax

        if sampling is not None and not isinstance(sampling, (bool, SamplingParams)):
            raise ValueError("ContinuousBatchDecoder: sampling must be None, a bool or the default SamplingParams, got "
                             f"{type(sampling).__name__}")
        if sampling is not None and sampling is not False and sample_fn is not None \
                and not isinstance(sample_fn, RequestSampler):
            raise ValueError("ContinuousBatchDecoder: sampling= needs a RequestSampler (or no sample_fn: one is built), "
                             "an ordinary sample_fn treats the batch as one request")
        self.default_sampling = (sampling if isinstance(sampling, SamplingParams) else SamplingParams()).check()
        self.module = module
        if prefill_chunk is not None and (not isinstance(prefill_chunk, int) or isinstance(prefill_chunk, bool)
                                          or prefill_chunk <= 0 or prefill_chunk % 32):
            raise ValueError(f"ContinuousBatchDecoder: prefill_chunk must be a positive multiple of 32, got "
                             f"{prefill_chunk!r}")
        self.prefill_chunk = prefill_chunk
        self.wide_batch = bool(wide_batch)
        self.skinny_gemm = bool(skinny_gemm) or self.wide_batch
        self.kv_cache = check_kv_cache_scheme(kv_cache, "ContinuousBatchDecoder")
        page = check_page_size(page_size, "ContinuousBatchDecoder")
        B = int(max_batch)
        if B < 1 or max_pages < 1 or record_steps < 1:
            raise ValueError("ContinuousBatchDecoder: max_batch, max_pages and record_steps must be at least 1")
        limit = (gemm_ops.WIDE_MAX_ROWS if wide_batch else gemm_ops.SKINNY_MAX_ROWS if skinny_gemm
                 else gemm_ops.GEMV_MAX_ROWS)
        if use_cuda_graph and B > limit:
            raise ValueError(
                f"ContinuousBatchDecoder: use_cuda_graph"
                f"{' with wide_batch' if wide_batch else ' with skinny_gemm' if skinny_gemm else ''} supports at most "
                f"{limit} rows, got {B}: above that the linear layers run library GEMMs, whose algorithm choice under "
                "graph capture need not be the eager one; run without use_cuda_graph")
        self.attns = [m for m in module.modules() if isinstance(m, ParallelSelfAttention)]
        assert self.attns, "no attention layers"
        if self.kv_cache is not None:
            for a in self.attns:
                a.check_fp8_kv_cache()
        if prefill_chunk is not None:
            for a in self.attns:
                a.check_chunked_prefill()
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
        if sample_fn is None and sampling is not None and sampling is not False:
            sample_fn = RequestSampler(B, self.state.capacity, dev)
        self.request_sampling = isinstance(sample_fn, RequestSampler)
        if self.request_sampling:
            if sample_fn.max_batch != B or sample_fn.history < self.state.capacity \
                    or sample_fn.table.buf.device != self.tok.device:
                raise ValueError(f"ContinuousBatchDecoder: the RequestSampler must have {B} rows and a history of at "
                                 f"least max_pages * page_size = {self.state.capacity} on the model's device")
            sample_fn.clear()  # warm-up and capture run over parked rows: they draw nothing and advance nothing
        self.sample_fn = sample_fn if sample_fn is not None else sample_argmax
        self.record_steps = int(record_steps)
        self._slot = torch.zeros(1, dtype=torch.long, device=dev)
        # one parked step sizes the recording ring (vocabulary, logits dtype) and warms the lazy module state
        with torch.no_grad(), gemm_ops.skinny_gemm(self.skinny_gemm, wide=self.wide_batch):
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
        with gemm_ops.skinny_gemm(self.skinny_gemm, wide=self.wide_batch):
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

    def _sampling_of(self, sampling: SamplingArg, n: int) -> list:
        """The checked ``SamplingParams`` of ``n`` requests being admitted: ``sampling`` is None (the decoder's
        default), one for all, or one per request."""
        from .sample import per_request

        if not self.request_sampling:
            if sampling is not None:
                raise ValueError("ContinuousBatchDecoder: sampling= needs a decoder built with a RequestSampler "
                                 "(sample_fn=RequestSampler(...) or sampling=True)")
            return [None] * n
        return per_request(self.default_sampling if sampling is None else sampling, n, "ContinuousBatchDecoder")

    @contextlib.contextmanager
    def _row_taken(self, row: int) -> Any:
        """Around the end of an admission, from the sampler's ``set_row`` to the request's record: if it raises, the
        sampler's row is parked again, so that no active table row stays over a decoder row without a request."""
        try:
            yield
        except BaseException:
            if self.request_sampling:
                self.sample_fn.clear_row(row)
            raise

    def _first_token(self, row: int, last: torch.Tensor, params: Any, prompt: Sequence[int]) -> torch.Tensor:
        """The request's first token ``[1, 1]`` from its prefill logits ``last [1, 1, V]``; with a ``RequestSampler`` the
        row's table entry is filled first and the draw runs on the one-row slice."""
        if not self.request_sampling:
            return self.sample_fn(last).reshape(1, 1).to(torch.long)
        self.sample_fn.set_row(row, params, prompt)
        return self.sample_fn.first(row, last).reshape(1, 1)

    def admit(self, row: int, input_tokens: Sequence[int], max_tokens: int, index: Any = None,
              sampling: SamplingArg = None) -> _Request:
        """Row ``row`` takes a request: the prompt is prefilled (eager, alone), its K/V copied into freshly allocated
        pages, the row's device state set and its first token drawn with one ``sample_fn`` call on the prefill logits.
        ``ValueError`` for a request that cannot fit ``max_pages`` pages or the model's sequence length, ``RuntimeError``
        naming the pool size when the pool lacks the prompt's pages -- both before anything is written.  ``sampling``
        (with a ``RequestSampler``): the request's ``SamplingParams``; None takes the decoder's default."""
        if self.prefill_chunk is not None:
            req = self.admit_many([row], [input_tokens], [max_tokens], sampling=sampling)[0]
            req.index = index
            return req
        n = len(input_tokens)
        self._check_request(row, n, max_tokens)
        params = self._sampling_of(sampling, 1)[0]
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
            with self._row_taken(row):
                first = self._first_token(row, last, params, input_tokens)
                self.state.assign(row, pages, n)
                self.tok[row : row + 1].copy_(first)
                req = _Request(index, n, int(max_tokens), pages)
                req.tokens.append(int(first.item()))
                req.logits.append(last.reshape(1, -1))
                self.rows[row] = req
        return req

    def _check_request(self, row: int, n: int, max_tokens: int) -> None:
        """``ValueError`` for a request that row ``row`` cannot take; nothing is changed."""
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

    def admit_many(self, rows: Sequence[int], prompts: Sequence[Sequence[int]],
                   max_tokens: Union[int, Sequence[int]], sampling: SamplingArg = None) -> list[_Request]:
        """Batched admission (requires ``prefill_chunk=C``): rows ``rows[i]`` take the requests (``prompts[i]``,
        ``max_tokens[i]``; one int serves all).  Every request is checked and all pages are allocated first -- a
        ``ValueError`` or the ``RuntimeError`` of an exhausted pool leaves everything as it was.  Pass j then forwards
        chunk j (at most C tokens, from position j * C) of every prompt that still has one, packed as one ``ChunkPass``
        of that many segments whose K/V go straight into the pages; a finished prompt drops out of the later passes, and
        its last-token logits are kept from the pass in which it ends.  Activations are those of one pass: at most
        ``len(rows) * C`` tokens.  After the last pass ``sample_fn`` is called once per request, in the order given --
        the calls of admitting the requests one by one -- and the rows' device state is set.  Until then the rows stay
        parked, so the captured step is not disturbed (``captures`` stays 1).  If a pass raises, all pages of the call
        are freed and the rows re-parked.  ``sampling`` (with a ``RequestSampler``): one ``SamplingParams`` for all or
        one per request; None takes the decoder's default."""
        if self.prefill_chunk is None:
            raise ValueError("ContinuousBatchDecoder.admit_many: batched admission needs prefill_chunk")
        rows, toks = [int(r) for r in rows], [list(p) for p in prompts]
        limits = [int(max_tokens)] * len(rows) if isinstance(max_tokens, int) else [int(m) for m in max_tokens]
        if not (len(rows) == len(toks) == len(limits)) or len(set(rows)) != len(rows):
            raise ValueError("ContinuousBatchDecoder.admit_many: one distinct row, prompt and max_tokens per request")
        if not rows:
            return []
        for row, t, m in zip(rows, toks, limits):
            self._check_request(row, len(t), m)
        params = self._sampling_of(sampling, len(rows))
        need = [-(-(len(t) + 1) // self.page_size) for t in toks]
        taken = self.allocator.alloc(sum(need))  # RuntimeError before anything is written
        pages = [taken[sum(need[:i]) : sum(need[: i + 1])] for i in range(len(rows))]
        C, st = self.prefill_chunk, self.state
        dev = st.pos.device
        settings = InferenceSettings(use_cache=True, reset_cache=False, cache_index=0, embedding_layers=[-1])
        last: list[Any] = [None] * len(rows)
        with torch.no_grad():
            try:
                for start in range(0, max(len(t) for t in toks), C):
                    segs = [(i, min(C, len(t) - start)) for i, t in enumerate(toks) if len(t) > start]
                    st.chunk = ChunkPass([(pages[i], start, m) for i, m in segs], self.max_pages, dev,
                                         ids=[tok for i, m in segs for tok in toks[i][start : start + m]])
                    with gemm_ops.skinny_gemm(self.skinny_gemm, wide=self.wide_batch):
                        out = self.module.forward(TextDatasetBatch(input_token_ids=st.chunk.ids.unsqueeze(0),
                                                                   position_ids=st.chunk.pos.unsqueeze(0),
                                                                   inference_settings=settings))
                    end = 0
                    for i, m in segs:
                        end += m
                        if start + m == len(toks[i]):  # the prompt ends in this pass
                            last[i] = out.activations[:, end - 1 : end, :].clone()
            except BaseException:
                for row in rows:
                    st.park(row)
                    if self.request_sampling:
                        self.sample_fn.clear_row(row)
                self.allocator.free(taken)
                raise
            finally:
                st.chunk = None
            reqs = []
            for i, row in enumerate(rows):
                with self._row_taken(row):
                    first = self._first_token(row, last[i], params[i], toks[i])
                    st.assign(row, pages[i], len(toks[i]))
                    self.tok[row : row + 1].copy_(first)
                    req = _Request(None, len(toks[i]), limits[i], pages[i])
                    req.tokens.append(int(first.item()))
                    req.logits.append(last[i].reshape(1, -1))
                    self.rows[row] = req
                reqs.append(req)
        return reqs

    def release(self, row: int) -> Optional[_Request]:
        """The row's pages go back to the free list and the row is parked; returns the request it held."""
        req = self.rows[row]
        if req is None:
            return None
        self.allocator.free(req.pages)
        self.state.park(row)
        if self.request_sampling:
            self.sample_fn.clear_row(row)
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
              check_every: int = 8, sampling: SamplingArg = None) -> list[tuple[list[int], torch.Tensor]]:
        """Runs ``requests`` = [(prompt tokens, max_tokens), ...] to completion, in arrival order: free rows are filled,
        all rows step, and every ``check_every`` steps (fewer when a row would pass its ``max_tokens``) the recorded
        tokens are read back; a request is cut at its first stop token or its ``max_tokens``, its row released and
        refilled.  Returns (tokens, logits ``[len(tokens), V]``) per request, in request order.  ``sampling`` (with a
        ``RequestSampler``): one ``SamplingParams`` for all or one per request."""
        params = self._sampling_of(sampling, len(requests))
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
            # batched admission: with prefill_chunk, several free rows and several waiting requests go in together
            while self.prefill_chunk is not None and len(self.free_rows) > 1 and len(requests) - nxt > 1:
                free = self.free_rows[: len(requests) - nxt]
                batch = requests[nxt : nxt + len(free)]
                reqs = self.admit_many(free, [t for t, _ in batch], [m for _, m in batch],
                                       sampling=params[nxt : nxt + len(free)] if self.request_sampling else None)
                for row, req in zip(free, reqs):
                    req.index = nxt
                    nxt += 1
                    if over(req):  # done with the prefill's token
                        finish(row)
            for row in self.free_rows:
                while nxt < len(requests) and self.rows[row] is None:
                    toks, mt = requests[nxt]
                    req = self.admit(row, toks, mt, index=nxt, sampling=params[nxt])
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
