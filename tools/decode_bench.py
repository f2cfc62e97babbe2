"""Batch-1 decode latency on one GPU: eager cached generation vs HIP-graph-captured decoding, greedy or sampled.

    python tools/decode_bench.py [--model llama2_7b] [--prompt 128] [--tokens 64] [--sampler T,K,P | torch:T,K,P]
                                 [--weights fp8_e4m3 | mxfp4 | bf16,fp8_e4m3,mxfp4 [--lm-head]] [--batch B [--skinny]]
                                 [--kv-cache bf16,fp8_e4m3 [--rounds N]] [--paged 0,64] [--continuous N]

``--batch B`` times batched generation instead (``generate_batch`` / ``BatchDecoder``): B random prompts of lengths
``prompt, prompt - 7, prompt - 14, ...`` decoded together; ms per step, tokens/s summed over the rows, and (B <= 4:
the graph limit) the captured loop and ``graph_tokens_equal_eager``.  ``--skinny`` passes ``skinny_gemm=True`` to
``batch_decoder``: the MFMA weight-streaming kernels (``csrc/kernels/skinny.hip``) and a graph limit of 16 rows.

``--weights fp8_e4m3`` decodes the model after ``quantize_weights()`` (FP8 weight-only decoding; ``--lm-head`` includes
the LM head); ``weights_gib`` and ``graph_gb_per_s`` then count what one decode step streams (the FP8 copies in place of
their bf16 parameters).  ``--weights mxfp4`` does the same with the MXFP4 copies (``quantize_weights("mxfp4")``).  A comma
list such as ``bf16,fp8_e4m3,mxfp4`` measures the formats alternately in this process, ``--rounds`` times, one JSON line
each: the model is re-quantised in place before each measurement (``bf16`` after a quantised format drops the copies and
decodes from the parameters, which then hold dequantised values: the same kernels and bytes as a fresh bf16 model).

``--kv-cache fp8_e4m3`` (with ``--batch``) decodes over the FP8 KV cache (``generate_batch(kv_cache=...)``); a comma
list such as ``bf16,fp8_e4m3`` measures the settings alternately in this process, ``--rounds`` times, one JSON line
each.  Every line carries ``kv_cache`` and ``kv_bytes_per_token`` (K and V of all layers).

``--paged PAGE`` (with ``--batch``) runs the static batch over the paged KV cache (``batch_decoder(page_size=PAGE)``); a
comma list such as ``0,64`` (0: the slab cache) measures the settings alternately in this process, ``--rounds`` times.

``--continuous N`` (with ``--batch B --skinny``, B the number of rows): a seeded stream of N requests (prompt lengths
``prompt - 7 * (i % 16)``, ``max_tokens`` uniform in ``--spread`` = 32,256, no stop tokens) served by continuous batching
over the paged cache (``ContinuousBatchDecoder.serve``, page size ``--paged`` or 64, one captured graph) and, for
comparison, by ``batch_decoder`` over the same requests in arrival-order groups of B, each group running to its longest
``max_tokens``.  Wall time covers prefills and decoding of both (graph captures excluded); tokens are the requested ones.
Also prints the KV memory each held: pages in use at the peak x bytes per page against B slabs of ``cap`` rows.

``--sampler 0.8,40,0.95`` decodes with the fused ``Sampler`` (temperature, top-k, top-p) in both loops;
``--sampler torch:0.8,40,0.95`` times the eager loop with the torch composition
``sample_temperature(top_p_transform(top_k_transform(x, k), p), T)``, which cannot be captured (no graph figures).

Random-init weights of the named preset; the prompt is random token ids.  Per-token time excludes the prefill
(eager: generate(N+1) - generate(1); graph: the replay loop alone, capture reported separately).  Prints one
JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="llama2_7b")
    p.add_argument("--prompt", type=int, default=128)
    p.add_argument("--tokens", type=int, default=64)
    p.add_argument("--num-layers", type=int, default=None)
    p.add_argument("--sampler", default=None, help="T,K,P: fused Sampler; torch:T,K,P: torch composition (eager only)")
    p.add_argument("--weights", default="bf16", help="bf16, fp8_e4m3 or mxfp4 (quantize_weights() first), or a comma list "
                   "measured alternately in this process, --rounds times")
    p.add_argument("--lm-head", action="store_true", help="with quantised --weights: quantise the LM head too")
    p.add_argument("--batch", type=int, default=0, help="B >= 1: time batched generation of B prompts")
    p.add_argument("--skinny", action="store_true", help="with --batch: skinny_gemm=True (MFMA kernels, graph up to B = 16)")
    p.add_argument("--kv-cache", default="bf16", help="with --batch: bf16, fp8_e4m3 (generate_batch(kv_cache=...)), or a "
                   "comma list measured alternately in this process (one JSON line per setting and round)")
    p.add_argument("--rounds", type=int, default=1, help="with --batch: repeat the --kv-cache list this many times")
    p.add_argument("--paged", default="0", help="with --batch: page size of the paged KV cache (0: slabs), or a comma list "
                   "measured alternately")
    p.add_argument("--continuous", type=int, default=0, help="with --batch B --skinny: serve N requests by continuous "
                   "batching and by static groups of B")
    p.add_argument("--spread", default="32,256", help="with --continuous: range of the requests' max_tokens")
    a = p.parse_args()
    a.page_list = [int(x) or None for x in a.paged.split(",")]
    a.kv_list = [None if k == "bf16" else k for k in a.kv_cache.split(",")]
    a.weight_list = a.weights.split(",")
    if any(w not in ("bf16", "fp8_e4m3", "mxfp4") for w in a.weight_list):
        raise SystemExit("--weights: bf16, fp8_e4m3, mxfp4 or a comma list of them")
    if a.kv_list != [None] and a.batch < 1:
        raise SystemExit("--kv-cache needs --batch (the single-sequence eager loop keeps a growing bf16 cache)")
    from scaling_amd.models import llama_architecture
    from scaling_amd.transformer.context.config import TransformerArchitectureConfig
    from scaling_amd.transformer.inference import (Sampler, TransformerInferenceModule, sample_argmax, sample_temperature,
                                                   top_k_transform, top_p_transform)
    from scaling_amd.transformer.model.model import get_transformer_layer_specs
    from scaling_amd.utils.gemm_tuning import enable_tuned_gemms

    enable_tuned_gemms("use")
    arch_d = llama_architecture(a.model, sequence_length=max(4096, a.prompt + a.tokens))
    if a.num_layers is not None:
        arch_d["num_layers"] = a.num_layers
    arch = TransformerArchitectureConfig.from_dict(arch_d)
    torch.manual_seed(0)
    m = TransformerInferenceModule(get_transformer_layer_specs(arch), devices=(0,))
    prompt = torch.randint(1, arch.vocab_size, (a.prompt,)).tolist()

    def set_weights(scheme):
        """Puts the model into ``scheme`` (in place) and returns quantize_weights()'s summary, None for bf16."""
        from scaling_amd.ops import quant

        a.weights = scheme
        if scheme == "bf16":
            for prm in m.parameters():
                quant.drop_w8(prm)
                quant.drop_w4(prm)
            return None
        return m.quantize_weights(scheme, include_lm_head=a.lm_head)

    sample_fn, graph_ok, mode = sample_argmax, True, "greedy"
    if a.sampler:
        spec = a.sampler.split(":")[-1].split(",")
        temp, top_k, top_p = float(spec[0]), int(spec[1]), float(spec[2])
        if a.sampler.startswith("torch:"):
            def sample_fn(x):
                return sample_temperature(top_p_transform(top_k_transform(x[0, -1], top_k), top_p)[None, None], temp)
            graph_ok, mode = False, f"torch composition T={temp} k={top_k} p={top_p}"
        else:
            sample_fn, mode = Sampler(temp, top_k, top_p, seed=0), f"fused sampler T={temp} k={top_k} p={top_p}"

    metric = "batch-1 greedy decode ms/token" if mode == "greedy" else "batch-1 sampled decode ms/token"

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t, r

    if a.batch >= 1:
        if not graph_ok:
            raise SystemExit("--batch needs a graph-safe sampler (greedy or T,K,P)")
        for _ in range(a.rounds):
            for scheme in a.weight_list:
                quantised = set_weights(scheme)
                for kv in a.kv_list:
                    if a.continuous:
                        continuous_bench(m, a, arch, sample_fn, timed, kv)
                        continue
                    for page in a.page_list:
                        batch_bench(m, a, arch, sample_fn, mode, timed, quantised, kv, page)
        return

    for _ in range(a.rounds):
        for scheme in a.weight_list:
            single_bench(m, a, arch, prompt, sample_fn, graph_ok, mode, metric, timed, set_weights(scheme))


def single_bench(m, a, arch, prompt, sample_fn, graph_ok, mode, metric, timed, quantised) -> None:
    """Batch 1: the eager loop and the captured loop in the model's current weight format."""
    from scaling_amd.transformer.inference.graph_decode import GraphDecoder

    m.generate(4, input_tokens=prompt, stop_tokens=[], sample_fn=sample_fn)  # warm-up (library handles, tables)
    t1, _ = timed(lambda: m.generate(1, input_tokens=prompt, stop_tokens=[], sample_fn=sample_fn))
    tn, eager = timed(lambda: m.generate(a.tokens + 1, input_tokens=prompt, stop_tokens=[], sample_fn=sample_fn))
    eager_ms = 1000.0 * (tn - t1) / a.tokens
    weights = sum(p.numel() * p.element_size() for p in m.parameters())
    extra = {"weights": a.weights}
    if quantised is not None:  # a decode step streams the quantised copies in place of their bf16 parameters
        weights = weights - quantised["bf16_bytes"] + quantised["quantized_bytes"]
        extra.update(lm_head=a.lm_head, quantised_tensors=quantised["tensors"], skipped=len(quantised["skipped"]),
                     bf16_gib_replaced=round(quantised["bf16_bytes"] / 2**30, 2))
    if not graph_ok:
        print(json.dumps({
            "metric": metric, "sampler": mode, "model": a.model, "layers": arch.num_layers,
            "prompt": a.prompt, "tokens": a.tokens, "eager_ms_per_token": round(eager_ms, 3),
            "weights_gib": round(weights / 2**30, 2), **extra,
        }), flush=True)
        return

    if hasattr(sample_fn, "reset"):
        sample_fn.reset(0)
    cur = m._pre_process_input(None, prompt, True)
    out = m.forward(cur)
    first = sample_fn(out.activations)
    dec = GraphDecoder(m, a.prompt, a.tokens + 1, first, sample_fn, out.activations[:, -1, :])
    tc, _ = timed(dec.capture)
    tg, (toks, _) = timed(lambda: dec.run([], check_every=a.tokens + 1))
    graph_ms = 1000.0 * tg / a.tokens
    same = toks == eager.completion_tokens
    print(json.dumps({
        "metric": metric, "sampler": mode, "model": a.model, "layers": arch.num_layers, "prompt": a.prompt,
        "tokens": a.tokens, "eager_ms_per_token": round(eager_ms, 3), "graph_ms_per_token": round(graph_ms, 3),
        "speedup": round(eager_ms / graph_ms, 2), "graph_capture_ms": round(1000.0 * tc, 1),
        "graph_tokens_equal_eager": same, "weights_gib": round(weights / 2**30, 2),
        "graph_gb_per_s": round(weights / (graph_ms * 1e-3) / 1e9, 1), **extra,
    }), flush=True)


def continuous_bench(m, a, arch, sample_fn, timed, kv=None) -> None:
    """``--continuous N``: total generated tokens / wall time of continuous batching against static groups of B."""
    import random

    B, N = a.batch, a.continuous
    page = a.page_list[0] or 64
    lo, hi = (int(x) for x in a.spread.split(","))
    rng = random.Random(0)
    gen = torch.Generator().manual_seed(1)
    reqs = [(torch.randint(1, arch.vocab_size, (max(1, a.prompt - 7 * (i % 16)),), generator=gen).tolist(),
             rng.randint(lo, hi)) for i in range(N)]
    total = sum(mt for _, mt in reqs)
    nkv = arch.attention_num_kv_heads or arch.num_attention_heads
    hd = arch.hidden_size // arch.num_attention_heads
    per_token = arch.num_layers * 2 * nkv * (2 * hd if kv is None else hd + 4)
    kw = dict(skinny_gemm=a.skinny, kv_cache=kv)
    graph = next(m.parameters()).is_cuda
    longest = max(len(p) + mt for p, mt in reqs)
    m.generate_continuous(4, input_tokens=[p for p, _ in reqs[:B]], max_batch=B, page_size=page, stop_tokens=[],
                          use_cuda_graph=graph, sample_fn=sample_fn, **kw)  # warm-up
    dec = m.continuous_decoder(B, page_size=page, max_pages=-(-longest // page), sample_fn=sample_fn, use_cuda_graph=graph,
                               **kw)
    tcont, out = timed(lambda: dec.serve(reqs, []))
    assert [len(t) for t, _ in out] == [mt for _, mt in reqs]
    tstat, cap_rows, steps_static = 0.0, 0, 0
    for g0 in range(0, N, B):
        group = reqs[g0 : g0 + B]
        mt = max(x for _, x in group)
        tp, sdec = timed(lambda: m.batch_decoder(mt, [p for p, _ in group], sample_fn, **kw))
        if graph:
            sdec.capture()
        tr, _ = timed(lambda: sdec.run([], check_every=mt))
        tstat += tp + tr
        steps_static += mt - 1
        cap_rows = max(cap_rows, len(group) * sdec.capacity)
    print(json.dumps({
        "metric": "continuous vs static batching, generated tokens/s", "requests": N, "rows": B, "model": a.model,
        "layers": arch.num_layers, "prompt": a.prompt, "max_tokens_range": [lo, hi], "tokens": total, "page": page,
        "kv_cache": kv or "bf16", "skinny_gemm": a.skinny,
        "continuous_s": round(tcont, 3), "continuous_tokens_per_s": round(total / tcont, 1), "continuous_steps": dec.steps_run,
        "static_s": round(tstat, 3), "static_tokens_per_s": round(total / tstat, 1), "static_steps": steps_static,
        "speedup": round(tstat / tcont, 2),
        "continuous_peak_pages": dec.allocator.peak_in_use + B,
        "continuous_kv_gib": round((dec.allocator.peak_in_use + B) * page * per_token / 2**30, 3),
        "static_kv_rows": cap_rows, "static_kv_gib": round(cap_rows * per_token / 2**30, 3),
    }), flush=True)


def batch_bench(m, a, arch, sample_fn, mode, timed, quantised, kv=None, page=None) -> None:
    """``--batch B``: per-step time of the batched decode loop (prefills and capture excluded); ``kv``: the KV cache
    scheme (None: bf16); ``page``: the paged cache's page size (None: slabs)."""
    from scaling_amd.ops.gemm import GEMV_MAX_ROWS, SKINNY_MAX_ROWS

    B, steps = a.batch, a.tokens
    if not hasattr(a, "prompts"):  # drawn once from the global stream (as ever): every setting and round decodes them
        a.prompts = [torch.randint(1, arch.vocab_size, (max(1, a.prompt - 7 * b),)).tolist() for b in range(B)]
    prompts = a.prompts
    nkv = arch.attention_num_kv_heads or arch.num_attention_heads
    hd = arch.hidden_size // arch.num_attention_heads
    kv_bytes = arch.num_layers * 2 * nkv * (2 * hd if kv is None else hd + 4)  # K and V, all layers, one token
    m.generate_batch(4, input_tokens=prompts, stop_tokens=[], sample_fn=sample_fn, skinny_gemm=a.skinny, kv_cache=kv,
                     page_size=page)  # warm-up
    dec = m.batch_decoder(steps + 1, prompts, sample_fn, skinny_gemm=a.skinny, kv_cache=kv, page_size=page)
    te, eager = timed(lambda: dec.run([], check_every=steps + 1))
    eager_ms = 1000.0 * te / steps
    weights = sum(p.numel() * p.element_size() for p in m.parameters())
    if quantised is not None:
        weights = weights - quantised["bf16_bytes"] + quantised["quantized_bytes"]
    res = {"metric": "batched decode ms/step", "batch": B, "sampler": mode, "model": a.model, "layers": arch.num_layers,
           "prompt": a.prompt, "tokens": steps, "weights": a.weights, "skinny_gemm": a.skinny, "kv_cache": kv or "bf16",
           "page_size": page or 0,
           "kv_bytes_per_token": kv_bytes, "eager_ms_per_step": round(eager_ms, 3),
           "eager_tokens_per_s": round(B * 1000.0 / eager_ms, 1), "weights_gib": round(weights / 2**30, 2)}
    if B <= (SKINNY_MAX_ROWS if a.skinny else GEMV_MAX_ROWS):
        dec = m.batch_decoder(steps + 1, prompts, sample_fn, skinny_gemm=a.skinny, kv_cache=kv, page_size=page)
        tc, _ = timed(dec.capture)
        tg, graph = timed(lambda: dec.run([], check_every=steps + 1))
        graph_ms = 1000.0 * tg / steps
        res.update(graph_ms_per_step=round(graph_ms, 3), graph_tokens_per_s=round(B * 1000.0 / graph_ms, 1),
                   graph_capture_ms=round(1000.0 * tc, 1),
                   graph_tokens_equal_eager=[g[0] for g in graph] == [e[0] for e in eager],
                   graph_gb_per_s=round(weights / (graph_ms * 1e-3) / 1e9, 1))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
