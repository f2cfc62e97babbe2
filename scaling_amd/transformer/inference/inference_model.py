"""Transformer inference (reference ``transformer/inference/inference_model.py``): checkpoint loading
with config + vocab, logits, hidden-state recording and greedy / sampled generation with or
without the KV cache."""
from __future__ import annotations

from pathlib import Path
from typing import Any, Callable, Optional, Sequence

import torch
import yaml

from ...core import BaseLayerIO, LayerSpec, PipePartitionMethod
from ...core.nn.linear.main_grad import invalidate_transposed_weights
from ...core.nn.parallel_module.inference_module import InferenceModule, RecorderSetting
from ..context.config import TransformerArchitectureConfig
from ..data import TextDatasetBatch
from ..data.inference_settings import InferenceSettings
from ..model.layers.base import TransformerLayerIO
from ..model.model import get_transformer_layer_specs
from ..tokenizer import Tokenizer
from .sample import sample_argmax


class CompletionOutput:
    def __init__(self, completion_text: Optional[str], completion_tokens: list[int], completion_logits: torch.Tensor):
        self.completion_text = completion_text
        self.completion_tokens = completion_tokens
        self.completion_logits = completion_logits


class TransformerInferenceModule(InferenceModule):
    def __init__(self, layer_specs: list[LayerSpec], devices: Sequence[Any] = (0,),
                 pipe_partition_method: PipePartitionMethod = PipePartitionMethod.UNIFORM,
                 pipe_partition_overwrite: Optional[list[int]] = None, tokenizer: Optional[Tokenizer] = None):
        super().__init__(layer_specs=layer_specs, devices=devices, pipe_partition_method=pipe_partition_method,
                         pipe_partition_overwrite=pipe_partition_overwrite)
        self.tokenizer = tokenizer

    @staticmethod
    def _parse_config_file(config_file: Path) -> TransformerArchitectureConfig:
        with open(config_file, "r") as f:
            d = yaml.safe_load(f)
        return TransformerArchitectureConfig.from_dict(d["transformer_architecture"])

    @classmethod
    def from_checkpoint(cls, checkpoint_dir: Path, devices: Sequence[Any] = (0,),
                        pipe_partition_method: PipePartitionMethod = PipePartitionMethod.UNIFORM,
                        pipe_partition_overwrite: Optional[list[int]] = None, config_file: Optional[Path] = None,
                        vocab_file: Optional[Path] = None,
                        weight_quantization: Optional[str] = None) -> "TransformerInferenceModule":
        """Weights, ``config.yml`` and ``vocab.json`` are expected in the checkpoint directory by default.
        ``weight_quantization`` (``"fp8_e4m3"`` or ``"mxfp4"``): ``quantize_weights`` is called after loading."""
        checkpoint_dir = Path(checkpoint_dir)
        config_file = config_file or checkpoint_dir / "config.yml"
        vocab_file = vocab_file or checkpoint_dir / "vocab.json"
        assert config_file.is_file(), "Config file not found"
        assert vocab_file.is_file(), "Vocab file not found"
        arch = cls._parse_config_file(config_file)
        model = cls(layer_specs=get_transformer_layer_specs(architecture_config=arch), devices=devices,
                    pipe_partition_method=pipe_partition_method, pipe_partition_overwrite=pipe_partition_overwrite,
                    tokenizer=Tokenizer.from_file(str(vocab_file)))
        model.load_checkpoint(checkpoint_dir)
        if weight_quantization is not None:
            model.quantize_weights(weight_quantization)
        return model

    def _quantization_groups(self, include_lm_head: bool) -> tuple[list[tuple[list[str], list[torch.Tensor]]], dict[str, str]]:
        """``([(names, weights sharing one input), ...], {name: reason it is never quantised})`` of this model."""
        from ...core.nn.mlp import ParallelSwiGLUMLP
        from ..model.layers import TransformerLayer, TransformerLMHead, TransformerLMHeadTied

        groups: list[tuple[list[str], list[torch.Tensor]]] = []
        skipped: dict[str, str] = {}

        def add(li: int, prefix: str, mods: list[tuple[str, torch.nn.Module]]) -> None:
            groups.append(([f"{li}.{prefix}{n}.weight" for n, _ in mods], [m.weight for _, m in mods]))

        for li, layer in enumerate(self._layers):
            topo = getattr(layer, "topology", None)
            if topo is not None and topo.config.model_parallel_size > 1:
                raise RuntimeError("quantize_weights: tensor parallelism (model_parallel_size > 1) is not supported")
            if isinstance(layer, TransformerLayer):
                att, mlp = layer.self_attention, layer.mlp
                if att.lora_config is not None and not att.lora_merged_state:
                    raise RuntimeError("quantize_weights: merge the LoRA adapters first (unmerged adapters read the "
                                       "bf16 weights they would be merged into)")
                if att.qkv_in_one:
                    add(li, "self_attention.", [("query_key_value", att.query_key_value)])
                else:
                    add(li, "self_attention.", [("query", att.query), ("key", att.key), ("value", att.value)])
                add(li, "self_attention.", [("dense", att.dense)])
                if isinstance(mlp, ParallelSwiGLUMLP):
                    add(li, "mlp.", [("dense_in", mlp.dense_in), ("siglu_weight", mlp.siglu_weight)])
                else:
                    add(li, "mlp.", [("dense_in", mlp.dense_in)])
                add(li, "mlp.", [("dense_out", mlp.dense_out)])
            elif isinstance(layer, TransformerLMHeadTied):
                if include_lm_head:
                    skipped[f"{li}.lm_head"] = "tied to the embedding"
            elif isinstance(layer, TransformerLMHead):
                if include_lm_head:
                    add(li, "", [("linear", layer.linear)])
        return groups, skipped

    def quantize_weights(self, scheme: str = "fp8_e4m3", include_lm_head: bool = False) -> dict:
        """Opt-in FP8 weight-only decoding (``ops/quant.py``, ``csrc/kernels/gemv.hip``).

        Every transformer layer's linear weights (q/k/v or fused qkv, attention dense, the MLP projections), and the
        LM head when asked (never a tied head, embeddings, norms or biases), get an OCP e4m3 copy with one
        power-of-two fp32 scale per output row, and the bf16 parameter is overwritten with the dequantised values:
        the copy is an exact encoding of the parameter.  Decode-sized linear layers (<= 4 rows) then stream the
        copy; the prefill GEMMs and every other path compute the same function from the bf16 parameters, which are
        kept (weights take 1.5x their bf16 memory: the mode trades memory for bytes per token).  Modifying a
        quantised parameter afterwards drops its copy (with a warning) and that layer decodes from bf16 again.

        ``scheme="mxfp4"`` (opt-in as well): the copy is OCP MXFP4 instead -- e2m1 codes, two per byte, in blocks of 32
        along K with one e8m0 power-of-two scale byte per block, 0.53125 bytes per weight --, again an exact encoding
        of the overwritten bf16 parameter, streamed by the MXFP4 forms of the same kernels (GEMV up to 4 rows, the MFMA
        kernel up to 16 inside ``skinny_gemm``); the weights then take about 1.27x their bf16 memory.  The model moves
        more than under FP8 (relative RMS weight error ~0.12).  It composes with everything the FP8 copies compose
        with (graph decoding, ``generate_batch``, ``skinny_gemm``, the FP8 / paged KV caches, continuous batching).

        Calling this again, with the same or the other scheme, re-quantises from the current parameter values and
        drops the old copies.

        On a CPU module the parameters are replaced by the dequantised values and the copies are kept but unused
        (the CPU path computes from the parameters).  Returns a summary: ``scheme``, ``tensors``, ``bf16_bytes``,
        ``quantized_bytes`` (the copies incl. scales, whatever the scheme; ``fp8_bytes`` is the same figure for
        ``fp8_e4m3`` and 0 otherwise), ``skipped`` (``{name: reason}``; a weight whose K is not a multiple of 16 --
        of 32 for ``mxfp4`` -- is skipped)."""
        from ...core.nn.linear.main_grad import adjacent_weights
        from ...ops import quant

        if scheme not in quant.SCHEMES:
            raise ValueError(f"quantize_weights: unknown scheme {scheme!r} (supported: "
                             f"{', '.join(repr(s) for s in quant.SCHEMES)})")
        piece = quant.MX_BLOCK if scheme == quant.SCHEME_MXFP4 else quant.PIECE
        if self.devices is None or len(self.devices) != 1:
            raise RuntimeError("quantize_weights: the model must sit on one device")
        groups, skipped = self._quantization_groups(include_lm_head)
        for names, weights in groups:
            for n, w in zip(names, weights):
                if w.dtype != torch.bfloat16:
                    raise RuntimeError(f"quantize_weights: bfloat16 models only ({n} is {w.dtype}); in fp16 the "
                                       "dequantised values would not be exact")
                if w.device != self.devices[0]:
                    raise RuntimeError(f"quantize_weights: {n} is on {w.device}, the model on {self.devices[0]}")
        for p in self.parameters():  # a parameter carries one copy: those of the other scheme go, head included
            (quant.drop_w8 if scheme == quant.SCHEME_MXFP4 else quant.drop_w4)(p)
        summary = {"scheme": scheme, "tensors": 0, "bf16_bytes": 0, "fp8_bytes": 0, "quantized_bytes": 0,
                   "skipped": skipped}
        for names, weights in groups:
            if any(w.dim() != 2 or w.shape[1] % piece for w in weights):
                for n, w in zip(names, weights):
                    skipped[n] = f"K is not a multiple of {piece}"
                    quant.drop_w8(w)  # (a copy of an earlier call in the other scheme)
                    quant.drop_w4(w)
                continue
            if len(weights) > 1:
                adjacent_weights(weights)  # the fused bf16 view's re-homing must precede the copies' version stamps
            b16, bq = quant.quantize_parameters(weights, scheme)
            summary["tensors"] += len(weights)
            summary["bf16_bytes"] += b16
            summary["quantized_bytes"] += bq
            if scheme == quant.SCHEME:
                summary["fp8_bytes"] += bq
        invalidate_transposed_weights()
        return summary

    def forward(self, x: BaseLayerIO) -> TransformerLayerIO:
        out = super().forward(x)
        assert isinstance(out, TransformerLayerIO)
        return out

    def _pre_process_input(self, input_text: Optional[str] = None, input_tokens: Optional[list[int]] = None,
                           process_for_cached_inference: bool = True) -> TextDatasetBatch:
        assert (input_text is None) ^ (input_tokens is None), "Either input_text or input_tokens needs to be provided"
        if input_text is not None:
            assert self.tokenizer is not None
            input_tokens = self.tokenizer.encode(input_text)
        settings = InferenceSettings(use_cache=process_for_cached_inference, reset_cache=True, cache_index=0,
                                     embedding_layers=[-1])
        return TextDatasetBatch(input_token_ids=torch.tensor(input_tokens).unsqueeze(0), inference_settings=settings)

    @staticmethod
    def _post_process_output(output: TransformerLayerIO) -> torch.Tensor:
        return output.activations.squeeze()

    def logits(self, input_text: Optional[str] = None, input_tokens: Optional[list[int]] = None) -> torch.Tensor:
        return self._post_process_output(self.forward(self._pre_process_input(input_text, input_tokens))).squeeze()

    def logits_with_hidden_state_recorder(self, input_text: Optional[str] = None, input_tokens: Optional[list[int]] = None,
                                          recorder_settings_per_layer: Optional[dict[int, RecorderSetting]] = None
                                          ) -> tuple[torch.Tensor, dict[int, dict[str, Any]]]:
        batch = self._pre_process_input(input_text, input_tokens)
        out, rec = super().forward_with_hidden_state_recorder(batch, recorder_settings_per_layer=recorder_settings_per_layer)
        assert isinstance(out, TransformerLayerIO)
        return self._post_process_output(out), rec

    def generate(self, max_tokens: int, input_text: Optional[str] = None, input_tokens: Optional[list[int]] = None,
                 sample_fn: Callable[[torch.Tensor], torch.Tensor] = sample_argmax,
                 stop_tokens: Optional[Sequence[int]] = None, use_cache: bool = True,
                 use_cuda_graph: bool = False, kv_cache: Optional[str] = None) -> CompletionOutput:
        """Completion text / tokens / logits for a prompt.  With the KV cache each step feeds only the new
        token (with its absolute position); without it the whole sequence is re-run.

        ``use_cuda_graph`` (KV cache, one GPU, flash attention, a graph-safe sampler: ``sample_argmax`` or
        ``sample.Sampler``): after the prefill, the decode step is captured once as a HIP graph and replayed per token
        (``graph_decode.GraphDecoder``) — same kernels and results as the eager loop, without its per-token
        launch and Python overhead.

        ``kv_cache="fp8_e4m3"`` (opt-in, with ``use_cuda_graph`` only): the decode steps keep K/V as e4m3 codes with
        one power-of-two scale per cached row (see ``generate_batch``).  The eager loop keeps its growing bf16 cache
        and raises ``ValueError`` if the argument is given."""
        from ...core.nn.attention.attention import check_kv_cache_scheme

        check_kv_cache_scheme(kv_cache, "generate")
        if kv_cache is not None and not use_cuda_graph:
            raise ValueError("generate: kv_cache needs use_cuda_graph=True (the eager loop keeps a growing bf16 KV cache); "
                             "generate_batch takes kv_cache with and without the graph")
        if stop_tokens is None:
            assert self.tokenizer is not None, "If no tokenizer is provided, a stop token needs to be set manually"
            stop_tokens = [self.tokenizer.eos_token_id]
        if hasattr(sample_fn, "reset"):
            sample_fn.reset(0)  # a seeded sampler (``sample.Sampler``) repeats its text from one call to the next
        cur = self._pre_process_input(input_text, input_tokens, process_for_cached_inference=use_cache)
        assert cur.input_token_ids is not None
        n_in = cur.input_token_ids.shape[-1]
        if use_cuda_graph:
            assert use_cache, "graph-captured decoding needs the KV cache"
            return self._generate_graph(cur, n_in, max_tokens, sample_fn, stop_tokens, kv_cache=kv_cache)
        settings = InferenceSettings(use_cache=use_cache, reset_cache=not use_cache, cache_index=0, embedding_layers=[-1])
        tokens: list[int] = []
        step_logits: list[torch.Tensor] = []
        out: Optional[TransformerLayerIO] = None
        for k in range(max_tokens):
            out = self.forward(cur)
            nxt = sample_fn(out.activations)
            tok = int(nxt.item())
            tokens.append(tok)
            if use_cache:
                step_logits.append(out.activations[:, -1, :])
                cur = TextDatasetBatch(input_token_ids=nxt.reshape(1, 1).cpu(), inference_settings=settings,
                                       position_ids=torch.tensor([[n_in + k]]))
            else:
                ids = torch.cat([cur.input_token_ids, nxt.reshape(1, 1).to(cur.input_token_ids.device)], dim=-1)
                cur = TextDatasetBatch(input_token_ids=ids, inference_settings=settings)
            if tok in stop_tokens:
                break
        if use_cache:
            logits = torch.cat(step_logits)
        else:
            assert out is not None
            logits = self._post_process_output(out)[n_in - 1 :]
        text = self.tokenizer.decode(tokens) if self.tokenizer is not None else None
        return CompletionOutput(completion_text=text, completion_tokens=tokens, completion_logits=logits)

    def batch_decoder(self, max_tokens: int, input_tokens: Sequence[Sequence[int]],
                      sample_fn: Callable[[torch.Tensor], torch.Tensor] = sample_argmax,
                      skinny_gemm: bool = False, kv_cache: Optional[str] = None, page_size: Optional[int] = None,
                      num_pages: Optional[int] = None) -> Any:
        """Prefills the prompts one at a time (prompt b under ``cache_index`` b), draws every row's first token with
        ONE ``sample_fn`` call on the stacked prefill logits and returns the ``batch_decode.BatchDecoder`` that decodes
        them together (not yet captured: call ``capture()`` for graph replay).  ``skinny_gemm``: its steps run inside
        ``ops.gemm.skinny_gemm()`` (the MFMA weight-streaming kernels for up to 16 rows, see ``generate_batch``).
        ``kv_cache``: None (bf16) or ``"fp8_e4m3"`` (see ``generate_batch``).  ``page_size``: the same static batch over
        the paged KV cache (``num_pages`` pages; see ``generate_batch``)."""
        from ...core.nn.attention.attention import ParallelSelfAttention, check_kv_cache_scheme, check_page_size
        from .batch_decode import BatchDecoder

        if page_size is not None:
            check_page_size(page_size, "generate_batch")

        if check_kv_cache_scheme(kv_cache, "generate_batch") is not None:  # refuse before the prefills run
            for m in self.modules():
                if isinstance(m, ParallelSelfAttention):
                    m.check_fp8_kv_cache()
        if len(input_tokens) == 0:
            raise ValueError("generate_batch: no prompts")
        if any(len(p) == 0 for p in input_tokens):
            raise ValueError("generate_batch: empty prompt")
        if max_tokens < 1:
            raise ValueError("generate_batch: max_tokens must be at least 1")
        if self.devices is None or len(self.devices) != 1:
            raise RuntimeError("generate_batch: the model must sit on one device")
        if hasattr(sample_fn, "reset"):
            sample_fn.reset(0)
        last = []
        for b, toks in enumerate(input_tokens):
            settings = InferenceSettings(use_cache=True, reset_cache=True, cache_index=b, embedding_layers=[-1])
            out = self.forward(TextDatasetBatch(input_token_ids=torch.tensor(list(toks)).unsqueeze(0),
                                                inference_settings=settings))
            last.append(out.activations[:, -1, :])
        prefill = torch.stack(last)  # [B, 1, V]
        first = sample_fn(prefill)
        return BatchDecoder(self, [len(p) for p in input_tokens], max_tokens, first, sample_fn, prefill,
                            skinny_gemm=skinny_gemm, kv_cache=kv_cache, page_size=page_size, num_pages=num_pages)

    def generate_batch(self, max_tokens: int, input_texts: Optional[Sequence[str]] = None,
                       input_tokens: Optional[Sequence[Sequence[int]]] = None,
                       sample_fn: Callable[[torch.Tensor], torch.Tensor] = sample_argmax,
                       stop_tokens: Optional[Sequence[int]] = None,
                       use_cuda_graph: bool = False, skinny_gemm: bool = False,
                       kv_cache: Optional[str] = None, page_size: Optional[int] = None) -> list[CompletionOutput]:
        """Completions for B prompts of any lengths, decoded together: one pass over the weights per step serves all
        B rows (``batch_decode.BatchDecoder``).  One device, always with the KV cache (flash attention kernel); the
        prompts are prefilled one at a time.  Stop tokens act per row: every row keeps stepping until all rows have
        stopped or ``max_tokens`` is reached, and each row's completion is cut at its first stop token.

        Greedy completions equal ``generate``'s per prompt up to the rounding of the batched kernels.  With a seeded
        ``sample.Sampler`` the row index is part of every draw, so a sampled batch does not repeat the text each
        prompt gets alone.

        ``use_cuda_graph`` replays the step as one HIP graph and needs ``B <= ops.gemm.GEMV_MAX_ROWS`` (4): above 4
        rows ``ops.gemm.linear`` uses a cached hipBLASLt plan in eager mode but torch's own path under capture, and
        the two need not pick the same algorithm, so graph tokens could not be kept equal to eager tokens.  The eager
        loop takes any B (rows > 4 run the library GEMMs and the unfused norm / SwiGLU kernels).

        ``skinny_gemm`` (opt-in) decodes ``ops.gemm.SKINNY_MIN_ROWS <= B <= 16`` rows on the MFMA weight-streaming
        kernels (``csrc/kernels/skinny.hip``; ``ops.gemm.skinny_gemm``), eager and graph alike, under the conditions of
        the GEMV paths (bf16 / fp16 model, optionally FP8 copies, one device, TP 1); ``use_cuda_graph`` then takes up to
        16 prompts.  Every row of those kernels is bitwise independent of the other rows.  The flag is inert off the
        GPU, and above 16 rows the eager loop runs the library path as without it.

        ``kv_cache="fp8_e4m3"`` (opt-in; default None, the bf16 cache): the decode steps keep K/V as OCP e4m3 codes with
        one fp32 power-of-two scale per cached row (one token of one kv head) -- ``hd + 4`` bytes instead of ``2 hd``
        -- written by the quantising RoPE + append kernel and read by the flash-decoding kernel
        (``BatchStaticKVCacheFP8``).  The prompts are prefilled against exact bf16 K/V and their rows quantised
        afterwards.  bf16 models on one device with the flash attention kernel; fp16, tensor parallelism and
        ``key_query_norm`` raise ``ValueError``.  It composes with ``quantize_weights`` and ``skinny_gemm``.

        ``page_size`` (opt-in, a multiple of 32; default None, one slab per row): the same static batch over the paged
        KV cache (``PagedKVCache``): each row owns ``ceil(length / page_size)`` pages of one pool instead of a slab of
        ``longest prompt + max_tokens`` rows, and gets a page whenever it grows into one.  Same kernels with one table
        lookup per 32-key tile; tokens and logits are the slab path's when ``longest prompt + max_tokens`` is a whole
        number of pages (the split plans then coincide).  ``generate_continuous`` refills finished rows on top of it."""
        from ...core.nn.attention.attention import check_kv_cache_scheme
        from ...ops.gemm import GEMV_MAX_ROWS, SKINNY_MAX_ROWS

        check_kv_cache_scheme(kv_cache, "generate_batch")

        if (input_texts is None) == (input_tokens is None):
            raise ValueError("generate_batch: give either input_texts or input_tokens")
        if input_texts is not None:
            assert self.tokenizer is not None
            input_tokens = [self.tokenizer.encode(t) for t in input_texts]
        assert input_tokens is not None
        if use_cuda_graph and skinny_gemm and len(input_tokens) > SKINNY_MAX_ROWS:
            raise ValueError(
                f"generate_batch: use_cuda_graph with skinny_gemm supports at most {SKINNY_MAX_ROWS} prompts, got "
                f"{len(input_tokens)}: above that the linear layers run library GEMMs, whose algorithm choice under "
                "graph capture need not be the eager one; run without use_cuda_graph")
        if use_cuda_graph and not skinny_gemm and len(input_tokens) > GEMV_MAX_ROWS:
            raise ValueError(
                f"generate_batch: use_cuda_graph supports at most {GEMV_MAX_ROWS} prompts, got {len(input_tokens)}: "
                "above that the linear layers use a cached hipBLASLt plan in eager mode but torch's own GEMM path "
                "under graph capture, which need not pick the same algorithm, so graph tokens could differ from "
                "eager tokens; run without use_cuda_graph")
        if stop_tokens is None:
            assert self.tokenizer is not None, "If no tokenizer is provided, a stop token needs to be set manually"
            stop_tokens = [self.tokenizer.eos_token_id]
        dec = self.batch_decoder(max_tokens, input_tokens, sample_fn, skinny_gemm=skinny_gemm, kv_cache=kv_cache,
                                 page_size=page_size)
        if use_cuda_graph:
            dec.capture()
        outs = []
        for tokens, logits in dec.run(stop_tokens):
            text = self.tokenizer.decode(tokens) if self.tokenizer is not None else None
            outs.append(CompletionOutput(completion_text=text, completion_tokens=tokens, completion_logits=logits))
        return outs

    def continuous_decoder(self, max_batch: int, page_size: int = 64, max_pages: int = 1,
                           num_pages: Optional[int] = None,
                           sample_fn: Callable[[torch.Tensor], torch.Tensor] = sample_argmax,
                           use_cuda_graph: bool = False, skinny_gemm: bool = False,
                           kv_cache: Optional[str] = None, record_steps: int = 8) -> Any:
        """The ``batch_decode.ContinuousBatchDecoder`` of this model for a serving loop (``admit`` / ``step`` /
        ``release``, or ``serve``): ``max_batch`` rows over a paged KV cache whose requests take at most ``max_pages``
        pages of ``page_size`` tokens; captured once when ``use_cuda_graph``.  See ``generate_continuous``."""
        from .batch_decode import ContinuousBatchDecoder

        if self.devices is None or len(self.devices) != 1:
            raise RuntimeError("generate_continuous: the model must sit on one device")
        return ContinuousBatchDecoder(self, max_batch, page_size=page_size, max_pages=max_pages, num_pages=num_pages,
                                      sample_fn=sample_fn, skinny_gemm=skinny_gemm, kv_cache=kv_cache,
                                      use_cuda_graph=use_cuda_graph, record_steps=record_steps)

    def generate_continuous(self, max_tokens: Any, input_texts: Optional[Sequence[str]] = None,
                            input_tokens: Optional[Sequence[Sequence[int]]] = None, max_batch: int = 4,
                            page_size: int = 64, num_pages: Optional[int] = None,
                            sample_fn: Callable[[torch.Tensor], torch.Tensor] = sample_argmax,
                            stop_tokens: Optional[Sequence[int]] = None, use_cuda_graph: bool = False,
                            skinny_gemm: bool = False, kv_cache: Optional[str] = None) -> list[CompletionOutput]:
        """Completions for N requests (N may exceed ``max_batch``) by continuous batching over a paged KV cache:
        ``max_batch`` rows share every decode step, and a row whose request reaches a stop token or its own
        ``max_tokens`` (an int, or one int per request) is refilled with the next request while the others go on
        (``batch_decode.ContinuousBatchDecoder.serve``).  Requests are admitted in order and returned in order.

        Each attention layer holds one pool of ``num_pages`` pages of ``page_size`` tokens (a multiple of 32); a request
        owns ``ceil(length / page_size)`` of them.  ``num_pages=None`` sizes the pool for ``max_batch`` sequences of the
        longest request (prompt + ``max_tokens``), plus one parking page per row.  A smaller pool raises
        ``RuntimeError`` when it runs out (there is no preemption).  ``use_cuda_graph`` captures the step once for the
        whole stream and has ``generate_batch``'s limits on ``max_batch`` (4, or 16 with ``skinny_gemm``); ``kv_cache``
        as in ``generate_batch``.  Greedy completions equal ``generate``'s per prompt up to the rounding of the batched
        kernels; with a seeded ``Sampler`` a draw depends on the row and the step a request happens to occupy."""
        if (input_texts is None) == (input_tokens is None):
            raise ValueError("generate_continuous: give either input_texts or input_tokens")
        if input_texts is not None:
            assert self.tokenizer is not None
            input_tokens = [self.tokenizer.encode(t) for t in input_texts]
        assert input_tokens is not None
        if len(input_tokens) == 0:
            raise ValueError("generate_continuous: no prompts")
        limits = [int(max_tokens)] * len(input_tokens) if isinstance(max_tokens, int) else [int(m) for m in max_tokens]
        if len(limits) != len(input_tokens):
            raise ValueError("generate_continuous: max_tokens must be an int or one int per request")
        if any(len(p) == 0 for p in input_tokens) or any(m < 1 for m in limits):
            raise ValueError("generate_continuous: empty prompt or max_tokens < 1")
        if stop_tokens is None:
            assert self.tokenizer is not None, "If no tokenizer is provided, a stop token needs to be set manually"
            stop_tokens = [self.tokenizer.eos_token_id]
        from ...core.nn.attention.attention import check_page_size

        check_page_size(page_size, "generate_continuous")
        longest = max(len(p) + m for p, m in zip(input_tokens, limits))
        dec = self.continuous_decoder(max_batch, page_size=page_size, max_pages=-(-longest // page_size),
                                      num_pages=num_pages, sample_fn=sample_fn, use_cuda_graph=use_cuda_graph,
                                      skinny_gemm=skinny_gemm, kv_cache=kv_cache)
        outs = []
        for tokens, logits in dec.serve(list(zip(input_tokens, limits)), stop_tokens):
            text = self.tokenizer.decode(tokens) if self.tokenizer is not None else None
            outs.append(CompletionOutput(completion_text=text, completion_tokens=tokens, completion_logits=logits))
        return outs

    def _generate_graph(self, prompt: TextDatasetBatch, n_in: int, max_tokens: int,
                        sample_fn: Callable[[torch.Tensor], torch.Tensor], stop_tokens: Sequence[int],
                        kv_cache: Optional[str] = None) -> CompletionOutput:
        from ...core.nn.attention.attention import ParallelSelfAttention
        from .graph_decode import GraphDecoder

        assert self.devices is not None and len(self.devices) == 1, "graph-captured decoding runs on one device"
        if kv_cache is not None:  # refuse before the prefill runs
            for m in self.modules():
                if isinstance(m, ParallelSelfAttention):
                    m.check_fp8_kv_cache()
        out = self.forward(prompt)  # prefill (reset_cache): fills each layer's KVCache
        first = sample_fn(out.activations)
        assert first.is_cuda, "graph-captured decoding needs a GPU"
        dec = GraphDecoder(self, n_in, max_tokens, first, sample_fn, out.activations[:, -1, :], kv_cache=kv_cache)
        dec.capture()
        tokens, logits = dec.run(stop_tokens)
        text = self.tokenizer.decode(tokens) if self.tokenizer is not None else None
        return CompletionOutput(completion_text=text, completion_tokens=tokens, completion_logits=logits)
