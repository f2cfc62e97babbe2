"""CPU checks of the fused sampler's pure-torch twin (``ops/sample.py``) and of ``Sampler``: the counter-based
uniform, the kept set against the reference composition ``top_p_transform(top_k_transform(x, k), p)``, the step
counter, and seeded ``generate``."""
import pytest
import torch

from scaling_amd.ops.sample import sample_distribution, sample_logits, sample_uniform
from scaling_amd.transformer.inference import Sampler, top_k_transform, top_p_transform

V = 1000
MARGIN = 1e-3


def test_uniform_twin_range_distinct_stable():
    steps = torch.arange(0, 512)
    rows = torch.arange(0, 64)
    u = sample_uniform(7, steps[:, None], rows[None, :])
    assert u.dtype == torch.float64 and u.shape == (512, 64)
    assert (u >= 0).all() and (u < 1).all()
    assert torch.equal(u * 2**24, (u * 2**24).round())  # 24-bit values: exact in the kernel's fp64 and in fp32
    # distinct across step (fixed row) and across row (fixed step); 24-bit hashes of a few hundred counters
    assert u[:, 0].unique().numel() == 512
    assert u[0, :].unique().numel() == 64
    assert u[:, 3].unique().numel() == 512 and u[5, :].unique().numel() == 64
    assert torch.equal(u, sample_uniform(7, steps[:, None], rows[None, :]))
    assert float(sample_uniform(7, 5, 3)) == float(u[5, 3])
    assert not torch.equal(u, sample_uniform(8, steps[:, None], rows[None, :]))
    # steps beyond 32 bits still change the draw
    assert float(sample_uniform(7, 5 + 2**32, 3)) != float(u[5, 3])
    assert 0.45 < float(u.mean()) < 0.55


def _margin_checked_p(x: torch.Tensor, k: int, p: float) -> float:
    """The p nearest to the nominal one (1e-3 grid, inside (0, 1)) at which the float64 cumulative mass at the cut token
    and at its predecessor both lie more than MARGIN away from it (the reference's fp32 softmax then takes the same
    cut).  That needs a cut token of probability above 2 * MARGIN: on a plain randn row of 1000 tokens without top-k
    only p below about 0.4 qualify, so the nominal 0.9 moves down there; with k = 10 it stays near 0.9."""
    y = x.double()
    if 0 < k < V:
        y = y.masked_fill(y < torch.topk(y, k)[0][-1], float("-inf"))
    cum = torch.cumsum(torch.softmax(torch.sort(y, descending=True)[0], dim=-1), dim=-1)
    for i in range(999):
        for q in (p + i * 1e-3, p - i * 1e-3):
            if not 0.0 < q < 0.9995:
                continue
            j = int((cum > q).to(torch.uint8).argmax())
            near = [abs(float(cum[j]) - q)] + ([abs(float(cum[j - 1]) - q)] if j > 0 else [])
            if min(near) > MARGIN:
                return q
    raise AssertionError("no margin-safe p found")


@pytest.mark.parametrize("p", [0.3, 0.9, 1.0])
@pytest.mark.parametrize("k", [1, 10, 1000, 0])
def test_kept_set_matches_reference_composition(k, p):
    torch.manual_seed(1234 + k)
    x = torch.randn(V, dtype=torch.float32)
    assert x.unique().numel() == V, "the comparison needs tie-free logits"
    if p < 1.0:
        p = _margin_checked_p(x, k, p)
        # the margin holds on these very inputs (asserted, not assumed)
        y = x.double() if not 0 < k < V else x.double().masked_fill(x.double() < torch.topk(x.double(), k)[0][-1], float("-inf"))
        cum = torch.cumsum(torch.softmax(torch.sort(y, descending=True)[0], dim=-1), dim=-1)
        j = int((cum > p).to(torch.uint8).argmax())
        assert abs(float(cum[j]) - p) > MARGIN and (j == 0 or abs(float(cum[j - 1]) - p) > MARGIN)
        assert 0.0 < p < 1.0
        print(f"k={k}: margin-checked p = {p:.4f}, cut at sorted position {j}")
    ref = x
    if k > 0:
        ref = top_k_transform(ref, k)
    if p < 1.0:
        ref = top_p_transform(ref, p)
    ref_kept = torch.isfinite(ref)

    kept, cdf, cut = sample_distribution(x[None, :], 1.0, k, p)
    assert torch.equal(kept[0], ref_kept)
    assert float(cdf[0, -1]) == pytest.approx(1.0, abs=1e-12)
    # through the public op: info's kept count, and the draws themselves
    n = 4096
    rows = x[None, :].expand(n, V)
    tokens, info = sample_logits(rows, 0, 11, temperature=100.0, top_k=k, top_p=p, want_info=True)
    assert tokens.dtype == torch.long and info.dtype == torch.int32
    assert int(info[0, 0]) == int(ref_kept.sum()) and bool((info[:, 0] == info[0, 0]).all())
    assert float(info[0, 1:].view(torch.float32)) == float(cut[0])
    drawn = torch.zeros(V, dtype=torch.bool)
    drawn[tokens] = True
    assert not bool((drawn & ~ref_kept).any()), "a token outside the reference's kept set was drawn"
    if int(ref_kept.sum()) <= 10:  # T = 100 makes the kept tokens near-uniform: 4096 draws exhaust at most 10 of them
        assert torch.equal(drawn, ref_kept)


def test_sampler_counter_and_seeds():
    torch.manual_seed(0)
    logits = torch.randn(1, 3, V)
    s = Sampler(temperature=1.0, top_k=0, top_p=1.0, seed=5)
    assert s.graph_safe and s.step == 0
    a = [int(s(logits)) for _ in range(64)]
    assert s.step == 64
    s.reset()
    assert s.step == 0
    assert [int(s(logits)) for _ in range(64)] == a
    s.reset(10)
    assert s.step == 10 and [int(s(logits)) for _ in range(5)] == a[10:15] and s.step == 15
    # a sampler with the same seed repeats, another seed does not
    assert [int(Sampler(seed=5)(logits))] == a[:1]
    t = Sampler(temperature=1.0, seed=6)
    assert [int(t(logits)) for _ in range(64)] != a
    # only the last position is sampled, one token per batch row
    two = Sampler(seed=5)(torch.randn(2, 3, V))
    assert two.shape == (2,)
    with pytest.raises(ValueError):
        Sampler(temperature=0.0)


def test_cpu_generate_repeats_with_one_sampler():
    from scaling_amd.transformer.context.config import TransformerArchitectureConfig
    from scaling_amd.transformer.inference import TransformerInferenceModule
    from scaling_amd.transformer.model.model import get_transformer_layer_specs

    arch = TransformerArchitectureConfig(
        vocab_size=256, hidden_size=256, num_layers=3, num_attention_heads=4, sequence_length=128, norm_type="rms",
        mlp_type="swiglu", mlp_factor=2.0, precision="float32", attention_num_kv_heads=2, attention_qkv_in_one=False,
        relative_position_embedding_type="rotary_complex", masked_softmax={"kernel": "torch"})
    torch.manual_seed(0)
    m = TransformerInferenceModule(get_transformer_layer_specs(arch), devices=("cpu",))
    prompt = [3, 17, 42, 99, 5, 7, 11]
    s = Sampler(0.8, 40, 0.95, seed=1)
    one = m.generate(12, input_tokens=prompt, stop_tokens=[], sample_fn=s)
    assert s.step == 12
    two = m.generate(12, input_tokens=prompt, stop_tokens=[], sample_fn=s)
    assert one.completion_tokens == two.completion_tokens and len(one.completion_tokens) == 12
    other = m.generate(12, input_tokens=prompt, stop_tokens=[], sample_fn=Sampler(0.8, 40, 0.95, seed=2))
    assert other.completion_tokens != one.completion_tokens
