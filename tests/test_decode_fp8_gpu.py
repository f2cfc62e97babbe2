"""FP8 weight-only decoding end to end (``TransformerInferenceModule.quantize_weights``) on the small Llama-layout
model of ``tests/test_gpu_e2e.py``: graph decoding equals eager decoding, the FP8 kernels are the ones taken, the logits
follow a never-quantised twin that carries the dequantised weights, and a modified weight falls back to bf16."""
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from scaling_amd.ops import quant  # noqa: E402
from scaling_amd.ops._ext import ext  # noqa: E402

PROMPT = [3, 17, 42, 99, 5, 7, 11]
LAYERS = 2
W8 = ("gemv_w8", "gemv_w8_residual", "gemv_w8_swiglu", "gemv_w8_norm")
BF16 = ("gemv", "gemv_residual", "gemv_swiglu", "gemv_norm", "gemv_norm_rope")


def _model(**kw):
    from scaling_amd.transformer.context.config import TransformerArchitectureConfig
    from scaling_amd.transformer.inference import TransformerInferenceModule
    from scaling_amd.transformer.model.model import get_transformer_layer_specs

    cfg = dict(vocab_size=256, hidden_size=256, num_layers=LAYERS, num_attention_heads=4, sequence_length=128,
               norm_type="rms", mlp_type="swiglu", mlp_factor=2.0, precision="bfloat16", attention_num_kv_heads=2,
               attention_qkv_in_one=False, relative_position_embedding_type="rotary_complex",
               masked_softmax={"kernel": "flash_attention"}, attention_bias=False, mlp_bias=False)
    cfg.update(kw)
    torch.manual_seed(0)
    return TransformerInferenceModule(get_transformer_layer_specs(TransformerArchitectureConfig(**cfg)), devices=(0,))


def _twin_of(m, **kw):
    """A never-quantised module carrying m's (dequantised) weights."""
    t = _model(**kw)
    with torch.no_grad():
        for (n, p), (n2, p2) in zip(m.named_parameters(), t.named_parameters()):
            assert n == n2
            p2.copy_(p)
    assert not any(hasattr(p, "_sa_w8") for p in t.parameters())
    return t


@pytest.fixture(scope="module")
def pair():
    """(quantised model, never-quantised twin on the dequantised weights, the twin's greedy tokens)."""
    m = _model()
    info = m.quantize_weights()
    assert info["tensors"] == 7 * LAYERS and info["skipped"] == {}
    t = _twin_of(m)
    greedy = t.generate(20, input_tokens=PROMPT, stop_tokens=[], use_cache=True).completion_tokens
    return m, t, greedy


def _count(monkeypatch, names):
    calls: dict = {}
    mod = ext()
    for name in names:
        fn = getattr(mod, name)

        def wrapped(*a, _fn=fn, _name=name, **k):
            out = _fn(*a, **k)
            calls[_name] = calls.get(_name, 0) + (out is not None)
            return out

        monkeypatch.setattr(mod, name, wrapped)
    return calls


def test_fp8_graph_decode_matches_eager(pair):
    from scaling_amd.transformer.inference import Sampler

    m = pair[0]
    for kw in ({}, {"sample_fn": Sampler(0.8, 40, 0.95, seed=1)}):
        eager = m.generate(20, input_tokens=PROMPT, stop_tokens=[], use_cache=True, **kw)
        graph = m.generate(20, input_tokens=PROMPT, stop_tokens=[], use_cache=True, use_cuda_graph=True, **kw)
        assert len(eager.completion_tokens) == 20
        assert graph.completion_tokens == eager.completion_tokens, (graph.completion_tokens, eager.completion_tokens)
        torch.testing.assert_close(graph.completion_logits.float().cpu(), eager.completion_logits.float().cpu(),
                                   rtol=1e-2, atol=1e-2)
        again = m.generate(20, input_tokens=PROMPT, stop_tokens=[], use_cache=True, use_cuda_graph=True, **kw)
        assert again.completion_tokens == graph.completion_tokens
    assert all(quant.w8_of(p) is not None for p in m.parameters() if hasattr(p, "_sa_w8"))


@pytest.mark.parametrize("graph", [False, True])
def test_fp8_kernels_are_taken(pair, monkeypatch, graph):
    """Per layer and decode step: q/k/v and gate/up through gemv_w8_norm, the attention output projection through
    gemv_w8, down + residual through gemv_w8_residual; no bf16 GEMV of any kind in the decode steps."""
    m = pair[0]
    steps = 4  # generate(5): the prefill and 4 decode steps (eager), one captured step (graph)
    calls = _count(monkeypatch, W8 + BF16)
    m.generate(steps + 1, input_tokens=PROMPT, stop_tokens=[], use_cache=True, use_cuda_graph=graph)
    n = LAYERS * (1 if graph else steps)  # a captured step is traced once (plus any warm-up runs)
    assert calls.get("gemv_w8_norm", 0) >= 2 * n and calls.get("gemv_w8_residual", 0) >= n, calls
    assert calls.get("gemv_w8", 0) >= n, calls
    assert all(calls.get(k, 0) == 0 for k in ("gemv_norm", "gemv_residual", "gemv_swiglu", "gemv_norm_rope")), calls
    # (ext().gemv still serves the tied, never-quantised head of this model)


def test_fp8_lm_head_is_counted(monkeypatch):
    m = _model(weight_tying=False)
    info = m.quantize_weights(include_lm_head=True)
    assert info["tensors"] == 7 * LAYERS + 1
    calls = _count(monkeypatch, W8 + BF16)
    steps = 3
    m.generate(steps + 1, input_tokens=PROMPT, stop_tokens=[], use_cache=True)
    assert calls.get("gemv_w8", 0) >= (LAYERS + 1) * steps, calls  # o-projection per layer + the head
    assert all(calls.get(k, 0) == 0 for k in BF16), calls


def _teacher_forced(m, tokens):
    """Prefill logits [n_in, V] and the logits of every decode step fed with ``tokens`` (generate()'s eager loop)."""
    from scaling_amd.transformer.data import TextDatasetBatch
    from scaling_amd.transformer.data.inference_settings import InferenceSettings

    out = m.forward(m._pre_process_input(None, PROMPT, process_for_cached_inference=True))
    prefill = out.activations[0].clone()
    settings = InferenceSettings(use_cache=True, reset_cache=False, cache_index=0, embedding_layers=[-1])
    steps = []
    for k, tok in enumerate(tokens):
        cur = TextDatasetBatch(input_token_ids=torch.tensor([[tok]]), inference_settings=settings,
                               position_ids=torch.tensor([[len(PROMPT) + k]]))
        steps.append(m.forward(cur).activations[:, -1, :].clone())
    return prefill, torch.cat(steps)


def test_fp8_teacher_forced_logits_follow_the_twin(pair):
    m, t, greedy = pair
    pa, sa = _teacher_forced(m, greedy)
    pb, sb = _teacher_forced(t, greedy)
    assert torch.equal(pa, pb)  # the prefill: same code, same weights
    assert sa.shape == sb.shape == (len(greedy), 256)
    diff = (sa.float() - sb.float()).abs().amax(dim=1)
    print("max |logit difference| per decode step:", [round(float(d), 4) for d in diff])
    torch.testing.assert_close(sa.float(), sb.float(), rtol=5e-2, atol=5e-2)  # every step, none left out


def test_fp8_stale_weight_falls_back(monkeypatch):
    m = _model()
    m.quantize_weights()
    w = m._layers[1].mlp.dense_out.weight
    with torch.no_grad():
        w.mul_(0.5)
    t = _twin_of(m)
    ref = t.generate(12, input_tokens=PROMPT, stop_tokens=[], use_cache=True)
    calls = _count(monkeypatch, W8 + BF16)
    quant._warned[0] = False
    with pytest.warns(RuntimeWarning, match="FP8 copy"):
        out = m.generate(12, input_tokens=PROMPT, stop_tokens=[], use_cache=True)
    assert not hasattr(w, "_sa_w8")
    # layer 1's down projection runs the bf16 kernel, the other layer's the FP8 one
    assert calls.get("gemv_residual", 0) == 11 and calls.get("gemv_w8_residual", 0) == 11 * (LAYERS - 1), calls
    tf_m, tf_t = _teacher_forced(m, ref.completion_tokens), _teacher_forced(t, ref.completion_tokens)
    assert torch.equal(tf_m[0], tf_t[0])
    torch.testing.assert_close(tf_m[1].float(), tf_t[1].float(), rtol=5e-2, atol=5e-2)
    assert len(out.completion_tokens) == 12
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m.generate(3, input_tokens=PROMPT, stop_tokens=[], use_cache=True)


def test_fp8_logit_drift_is_reported(pair):
    """Informational (no threshold): relative RMS difference of the logits between the original bf16 model and its
    quantised self."""
    orig = _model()
    a = orig.logits(input_tokens=PROMPT).float()
    b = pair[0].logits(input_tokens=PROMPT).float()
    rel = float((a - b).pow(2).mean().sqrt() / a.pow(2).mean().sqrt())
    print(f"relative RMS logit difference bf16 vs fp8_e4m3: {rel:.4f}")
    assert rel == rel and rel > 0  # the quantised model is a different (nearby) model
