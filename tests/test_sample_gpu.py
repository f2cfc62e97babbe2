"""MI355X checks of the fused top-k / top-p / temperature sampling kernel (``csrc/kernels/sample.hip``) against its
float64 torch twin (``ops.sample.sample_distribution``), and of ``Sampler`` inside eager and graph-captured decoding.

CDF slack ``EPS = 1e-4``: a hierarchical scan over at most 131072 elements with at most a few hundred sequential adds
per thread is off by under about 1e-5 of the total mass, the hardware exp2 by about 2^-21 relative; 1e-4 leaves an
order of magnitude of room and still rejects any off-by-one token of probability above 2e-4.  Measured on an MI355X
over the whole matrix of ``test_kernel_matches_oracle`` (420 cases of 16 steps): no draw left its interval at all
(worst excursion -5e-10, i.e. inside); the kernel accumulates the draw in fp64."""

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-4
MARGIN = 1e-3
STEPS = [0, 1, 2, 3, 5, 8, 13, 100, 101, 1000, 65535, 65536, 2**31, 2**32 + 1, 2**40, 2**62]
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def _ops():
    from scaling_amd.ops import sample

    return sample


def _resident_limit() -> int:
    from scaling_amd.ops._ext import ext

    return int(ext().sample_max_resident_vocab())


def _settings(V):
    return [(0, 1.0, 1.0), (1, 1.0, 1.0), (50, 1.0, 0.7), (0, 0.9, 1.0), (40, 0.95, 0.05), (0, 1e-6, 1.0), (V + 5, 1.0, 1.0)]


def _margin_ok(x, k, p):
    """Per row: the float64 mass (temperature 1, over what top-k kept) down to and including the oracle's cut value,
    and the mass strictly above it (the predecessor's inclusive mass), are both more than MARGIN away from p."""
    _, _, cut = _ops().sample_distribution(x, 1.0, k, p)
    xd = x.float().double()
    kk, _, _ = _ops().sample_distribution(x, 1.0, k, 1.0)
    e = torch.where(kk, torch.exp(xd - xd.max(dim=-1, keepdim=True).values), torch.zeros_like(xd))
    z = e.sum(-1)
    ge = torch.where(xd >= cut[:, None], e, torch.zeros_like(e)).sum(-1) / z
    gt = torch.where(xd > cut[:, None], e, torch.zeros_like(e)).sum(-1) / z
    pf = float(torch.tensor(p, dtype=torch.float32))
    return ((ge - pf).abs() > MARGIN) & ((gt == 0) | ((gt - pf).abs() > MARGIN))


def _nearest_margin_p(x, k, p0):
    """The p closest to p0 (on a 1e-3 grid) at which every row has the margin.  The margin needs a cut token of
    probability above 2 * MARGIN, so on flat rows only small p qualify."""
    for i in range(999):
        for p in (p0 + i * 1e-3, p0 - i * 1e-3):
            if 0.0 < p < 0.9995 and bool(_margin_ok(x, k, p).all()):
                return p
    raise AssertionError("no p with the margin on these rows")


def _run_case(x, k, p, T, seed, steps=STEPS):
    """Draws at every step; returns device tensors (all-ok flag, worst CDF excursion, info, oracle kept count)."""
    ops = _ops()
    B, V = x.shape
    kept, cdf, cut = ops.sample_distribution(x, T, k, p)
    step = torch.zeros(1, dtype=torch.long, device=x.device)
    toks, info = [], None
    for s in steps:
        step.fill_(s)
        if info is None:
            t, info = ops.sample_logits(x, step, seed, T, k, p, want_info=True)
        else:
            t = ops.sample_logits(x, step, seed, T, k, p)
        toks.append(t)
    tok = torch.stack(toks)  # [S, B]
    u = ops.sample_uniform(seed, torch.tensor(steps, device=x.device)[:, None], torch.arange(B, device=x.device)[None, :])
    inb = (tok >= 0) & (tok < V)
    tc = tok.clamp(0, V - 1).t()  # [B, S]
    in_kept = kept.gather(1, tc).t()
    hi = cdf.gather(1, tc).t()
    lo = torch.where(tc > 0, cdf.gather(1, (tc - 1).clamp(min=0)), torch.zeros_like(hi.t())).t()
    exc = torch.maximum(lo - u, u - hi)
    ok = inb.all() & in_kept.all() & (exc <= EPS).all()
    cut_ok = (info[:, 1].contiguous().view(torch.float32).double() == cut).all()
    return ok, exc.max(), info, kept.sum(-1), cut_ok


def _vocab_sizes():
    return [1, 5, 64, 255, 1000, 32000, 32003, 128000, "limit", "limit+1"]


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("V", _vocab_sizes())
def test_kernel_matches_oracle(V, dtype):
    """Every draw lies in the oracle's kept set and its uniform inside the oracle's CDF interval of the returned
    token (+- EPS); info's kept count equals the oracle's for top-k alone, and with top-p wherever the margin holds."""
    if isinstance(V, str):
        V = _resident_limit() + (1 if V.endswith("+1") else 0)
    torch.manual_seed(V)
    base = (torch.randn(7, V + 13, device=DEV) * 3.0).to(DTYPES[dtype])
    results = []
    for B in (1, 7):
        x = base[:B, 3:3 + V]  # row stride V + 13 > V, rows not 16-byte aligned
        assert x.stride(0) > V or B == 1
        for (k, p, T) in _settings(V):
            ok, exc, info, n_kept, cut_ok = _run_case(x, k, p, T, seed=V + B)
            count_ok = info[:, 0] == n_kept
            if p < 1.0:
                count_ok = count_ok | ~_margin_ok(x, k, p)
                cut_ok = cut_ok | ~_margin_ok(x, k, p).all()
            results.append(((B, k, p, T), ok, exc, count_ok.all(), cut_ok))
    for case, ok, exc, count_ok, cut_ok in results:
        print(f"V={V} {dtype} B,k,p,T={case}: worst CDF excursion {float(exc):.3e}")
        assert bool(ok), (case, float(exc))
        assert bool(count_ok), ("kept count", case)
        assert bool(cut_ok), ("cut logit", case)


@pytest.mark.parametrize("V", [1000, 32000, 128000])
def test_kept_count_on_margin_checked_p(V):
    """fp32 rows, p moved until the float64 mass at the cut token and at its predecessor are more than 1e-3
    from it (asserted): info's kept count and cut logit equal the oracle's."""
    torch.manual_seed(V + 1)
    x = torch.randn(4, V, device=DEV) * 6.0  # peaked: the margin needs cut tokens of probability > 2e-3
    for k, p0 in [(0, 0.3), (0, 0.9), (40, 0.95), (10, 0.5)]:
        p = _nearest_margin_p(x, k, p0)
        assert bool(_margin_ok(x, k, p).all()) and 0.0 < p < 1.0
        ok, exc, info, n_kept, cut_ok = _run_case(x, k, p, 1.0, seed=3, steps=STEPS[:4])
        assert bool(ok), float(exc)
        assert torch.equal(info[:, 0].long(), n_kept) and bool(cut_ok), (k, p)


def test_edge_rows():
    ops = _ops()
    V = 1000
    # all logits equal: every token kept whatever the filters, draws follow the uniform CDF
    x = torch.full((3, V), 1.5, device=DEV)
    for k, p in [(0, 1.0), (10, 0.5)]:
        ok, exc, info, n_kept, cut_ok = _run_case(x, k, p, 1.0, seed=9)
        assert bool(ok) and bool((info[:, 0] == V).all()) and bool(cut_ok), float(exc)
    # one logit 60 above the rest: always returned
    for dt in DTYPES.values():
        x = torch.randn(5, V, device=DEV).to(dt)
        hot = torch.tensor([0, 1, 500, 998, 999], device=DEV)
        x[torch.arange(5), hot] = 60.0 + x.float().max().item()
        for k, p, T in [(0, 1.0, 1.0), (50, 0.9, 0.7)]:
            ok, exc, info, _, _ = _run_case(x, k, p, T, seed=2)
            assert bool(ok)
            step = torch.zeros(1, dtype=torch.long, device=DEV)
            for s in STEPS:
                step.fill_(s)
                assert torch.equal(ops.sample_logits(x, step, 2, T, k, p), hot)
    # half the row -inf: never returned, never counted
    x = torch.randn(4, V, device=DEV)
    dead = torch.rand(4, V, device=DEV) < 0.5
    dead[:, 0] = True
    x = x.masked_fill(dead, float("-inf"))
    for k, p, T in [(0, 1.0, 1.0), (750, 1.0, 1.0), (0, 0.999, 2.0), (600, 0.9, 0.05)]:
        ok, exc, info, n_kept, _ = _run_case(x, k, p, T, seed=4)
        assert bool(ok), float(exc)
        if p >= 1.0:
            assert torch.equal(info[:, 0].long(), (~dead).sum(-1)) and torch.equal(info[:, 0].long(), n_kept)
        step = torch.zeros(1, dtype=torch.long, device=DEV)
        for s in range(32):
            step.fill_(s)
            t = ops.sample_logits(x, step, 4, T, k, p)
            assert not bool(dead.gather(1, t[:, None]).any())
    # a row without a finite logit: token 0, nothing kept
    t, info = ops.sample_logits(torch.full((2, 77), float("-inf"), device=DEV), 0, 1, 1.0, 5, 0.9, want_info=True)
    assert t.tolist() == [0, 0] and info[:, 0].tolist() == [0, 0]


def test_heavy_ties_bf16_kept_count():
    """bf16 rows at V = 32000 quantised to quarter steps (tie groups of hundreds): the kept count is the
    tie-inclusive oracle's, for top-k alone and for margin-checked p."""
    torch.manual_seed(5)
    x = ((torch.randn(4, 32000, device=DEV) * 2.0) * 4).round().div(4).to(torch.bfloat16)
    assert x[0].unique().numel() < 200
    for k, p0 in [(50, 1.0), (1, 1.0), (5000, 1.0), (0, 0.9), (40, 0.5)]:
        p = p0
        if p < 1.0:
            p = _nearest_margin_p(x, k, p0)
            assert bool(_margin_ok(x, k, p).all()) and 0.0 < p < 1.0
        ok, exc, info, n_kept, cut_ok = _run_case(x, k, p, 1.0, seed=6)
        assert bool(ok), float(exc)
        assert torch.equal(info[:, 0].long(), n_kept) and bool(cut_ok), (k, p)
        if k == 50:
            assert bool((n_kept > 50).all())  # the tie-mates of the 50th value are in


def test_frequencies():
    ops = _ops()
    w = torch.tensor([0.06, 0.4, 0.005, 0.1, 0.0125, 0.2, 0.03, 0.08, 0.015, 0.04, 0.01, 0.0075, 0.02, 0.006, 0.009, 0.005],
                     dtype=torch.float64)
    w = w / w.sum()
    B = 65536
    logits = w.log().float().to(DEV)[None, :].expand(B, 16)
    for k in (0, 4):
        _, cdf, _ = ops.sample_distribution(logits[:1], 1.0, k, 1.0)
        prob = torch.diff(cdf[0], prepend=torch.zeros(1, dtype=torch.float64, device=DEV)).cpu()
        if k == 0:
            assert float(prob.max()) == pytest.approx(float(w.max()), rel=1e-6) and float(prob.min()) < 0.006
        else:
            assert int((prob > 0).sum()) == 4 and float(prob.sum()) == pytest.approx(1.0)
        tokens = ops.sample_logits(logits, 17, 123, 1.0, k, 1.0)
        counts = torch.bincount(tokens.cpu(), minlength=16).double()
        sd = torch.sqrt(B * prob * (1 - prob))
        dev = (counts - B * prob).abs()
        print("k", k, "counts", counts.tolist(), "z", (dev / sd.clamp(min=1e-9)).tolist())
        assert bool((dev <= 5 * sd).all()), (counts.tolist(), (B * prob).tolist())


def test_determinism():
    ops = _ops()
    torch.manual_seed(11)
    x = torch.randn(4096, 32000, device=DEV, dtype=torch.bfloat16) * 3
    step = torch.tensor([7], device=DEV)
    a = ops.sample_logits(x, step, 5, 0.8, 40, 0.95, want_info=True)
    b = ops.sample_logits(x, step, 5, 0.8, 40, 0.95, want_info=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[0].unique().numel() > 1000


def test_native_path_required(monkeypatch):
    """A GPU tensor never falls back to the torch path: without the extension the op raises."""
    from scaling_amd.ops import _ext

    def missing():
        raise RuntimeError("scaling_amd HIP extension is not built")

    monkeypatch.setattr(_ops(), "ext", missing)
    with pytest.raises(RuntimeError):
        _ops().sample_logits(torch.randn(1, 8, device=DEV), 0, 0)
    assert _ext.available()


@pytest.fixture(scope="module")
def tiny_model():
    from scaling_amd.transformer.context.config import TransformerArchitectureConfig
    from scaling_amd.transformer.inference import TransformerInferenceModule
    from scaling_amd.transformer.model.model import get_transformer_layer_specs

    arch = TransformerArchitectureConfig(
        vocab_size=256, hidden_size=256, num_layers=3, num_attention_heads=4, sequence_length=128, norm_type="rms",
        mlp_type="swiglu", mlp_factor=2.0, precision="bfloat16", attention_num_kv_heads=2, attention_qkv_in_one=False,
        relative_position_embedding_type="rotary_complex", masked_softmax={"kernel": "flash_attention"})
    torch.manual_seed(0)
    return TransformerInferenceModule(get_transformer_layer_specs(arch), devices=(0,))


PROMPT = [3, 17, 42, 99, 5, 7, 11]


def test_graph_decode_samples_like_eager(tiny_model):
    from scaling_amd.transformer.inference import Sampler

    m = tiny_model
    s = Sampler(0.8, 40, 0.95, seed=1)
    eager = m.generate(20, input_tokens=PROMPT, stop_tokens=[], sample_fn=s)
    graph = m.generate(20, input_tokens=PROMPT, stop_tokens=[], sample_fn=s, use_cuda_graph=True)
    assert graph.completion_tokens == eager.completion_tokens, (graph.completion_tokens, eager.completion_tokens)
    torch.testing.assert_close(graph.completion_logits.float().cpu(), eager.completion_logits.float().cpu(),
                               rtol=1e-2, atol=1e-2)
    again = m.generate(20, input_tokens=PROMPT, stop_tokens=[], sample_fn=s, use_cuda_graph=True)
    assert again.completion_tokens == graph.completion_tokens
    other = m.generate(20, input_tokens=PROMPT, stop_tokens=[], sample_fn=Sampler(0.8, 40, 0.95, seed=2), use_cuda_graph=True)
    assert other.completion_tokens != graph.completion_tokens
    greedy = m.generate(20, input_tokens=PROMPT, stop_tokens=[])
    assert greedy.completion_tokens != graph.completion_tokens  # the sampler does sample
    for cg in (False, True):
        top1 = m.generate(20, input_tokens=PROMPT, stop_tokens=[], sample_fn=Sampler(top_k=1), use_cuda_graph=cg)
        assert top1.completion_tokens == greedy.completion_tokens
    # a stop token taken from position 5 of the sampled sequence cuts both runs at the same place
    stops = [eager.completion_tokens[5]]
    e2 = m.generate(20, input_tokens=PROMPT, stop_tokens=stops, sample_fn=s)
    g2 = m.generate(20, input_tokens=PROMPT, stop_tokens=stops, sample_fn=s, use_cuda_graph=True)
    n = eager.completion_tokens.index(stops[0]) + 1
    assert e2.completion_tokens == eager.completion_tokens[:n] and g2.completion_tokens == e2.completion_tokens
    assert g2.completion_logits.shape[0] == n
