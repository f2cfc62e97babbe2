"""Paged KV cache decoders on the GPU: the static batch over the paged cache against the slab cache (bit for bit, eager and
under the graph), continuous batching against the same request in a static paged batch (bit for bit, whichever row and
neighbours it had), one capture for all admissions, the kernels taken, the errors.  Model and prompts are those of
``tests/batch_decode_common.py``."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from batch_decode_common import PROMPTS, make_model  # noqa: E402
from scaling_amd.ops._ext import ext  # noqa: E402
from scaling_amd.transformer.inference import Sampler  # noqa: E402

LAYERS = 2
FP8 = "fp8_e4m3"
PAGE = 32
STATIC_TOKENS = 63  # lengths 7, 1, 33, 12(, 9): cap = 33 + 63 = 96 = three pages, the slab's split plan
LIMITS = [5, 40, 12, 63, 20, 9]


@pytest.fixture(scope="module")
def model():
    return make_model(0, "bfloat16")


@pytest.fixture(scope="module")
def qmodel():
    m = make_model(0, "bfloat16")
    m.quantize_weights()
    return m


def _static(m, prompts, max_tokens, graph, **kw):
    dec = m.batch_decoder(max_tokens, prompts, **kw)
    if graph:
        dec.capture()
    out = dec.run([])
    return dec, [(t, lg.clone()) for t, lg in out]


def _bitwise(a, b, what):
    assert len(a) == len(b)
    for i, ((ta, la), (tb, lb)) in enumerate(zip(a, b)):
        assert ta == tb, (what, i, ta, tb)
        assert la.shape == lb.shape and torch.equal(la, lb), (what, i, (la.float() - lb.float()).abs().max().item())


@pytest.mark.parametrize("case", ["gemv4", "gemv4-sampled", "skinny5", "skinny5-sampled", "fp8kv3", "fp8weights4"])
def test_paged_static_batch_equals_slab_batch(model, qmodel, case):
    name, _, sampled = case.partition("-")
    m = qmodel if name == "fp8weights4" else model
    B = int(name[-1])
    kw = {}
    if name in ("skinny5", "fp8kv3"):
        kw["skinny_gemm"] = True
    if name == "fp8kv3":
        kw["kv_cache"] = FP8
    prompts = PROMPTS[:B]
    runs = {}
    for graph in (False, True):
        for page in (None, PAGE):
            if sampled:
                kw["sample_fn"] = Sampler(0.8, 40, 0.95, seed=1)
            dec, runs[graph, page] = _static(m, prompts, STATIC_TOKENS, graph, page_size=page, **kw)
            assert all(len(t) == STATIC_TOKENS for t, _ in runs[graph, page])
            if page is not None:
                # rows crossed the 32 and 64 boundaries at different steps: pages came one by one
                assert [len(p) for p in dec.pages] == [-(-(len(p) + STATIC_TOKENS) // PAGE) for p in prompts]
                assert dec.allocator.in_use == sum(len(p) for p in dec.pages)
    _bitwise(runs[False, PAGE], runs[False, None], "eager paged vs slab")
    _bitwise(runs[True, PAGE], runs[True, None], "graph paged vs slab")
    for (tg, _), (te, _) in zip(runs[True, PAGE], runs[False, PAGE]):
        assert tg == te  # graph tokens equal eager tokens


@pytest.fixture(scope="module")
def static_refs(model):
    """Request i decoded in a static paged batch of three (row 0; the next two prompts as neighbours), eager and graph."""
    refs = {}
    for graph in (False, True):
        for i, (p, n) in enumerate(zip(PROMPTS, LIMITS)):
            group = [p, PROMPTS[(i + 1) % 6], PROMPTS[(i + 2) % 6]]
            _, out = _static(model, group, n, graph, skinny_gemm=True, page_size=PAGE)
            refs[graph, i] = out[0]
    return refs


@pytest.mark.parametrize("graph", [False, True])
def test_continuous_equals_static_row_for_row(model, static_refs, graph):
    stop = static_refs[False, 3][0][17]  # request 3 (63 tokens allowed) stops early
    dec = model.continuous_decoder(3, page_size=PAGE, max_pages=3, skinny_gemm=True, use_cuda_graph=graph)
    pool = dec.allocator.free_pages
    assert pool == 9 and dec.captures == (1 if graph else 0)
    g0 = dec.graph
    handed, alloc = [], dec.allocator.alloc

    def logged(n):
        pages = alloc(n)
        handed.extend(pages)
        return pages

    dec.allocator.alloc = logged
    out = dec.serve(list(zip(PROMPTS, LIMITS)), [stop])
    assert dec.graph is g0 and dec.captures == (1 if graph else 0)  # six admissions, one graph
    assert dec.allocator.free_pages == pool and dec.free_rows == [0, 1, 2]
    assert len(handed) > len(set(handed))  # some refills landed on recycled pages
    worst = 0.0
    for i, (tokens, logits) in enumerate(out):
        rt, rl = static_refs[graph, i]
        cut = next((j + 1 for j, t in enumerate(rt) if t == stop), len(rt))
        assert tokens == rt[:cut], (i, tokens, rt[:cut])
        assert logits.shape == (cut, 256)
        worst = max(worst, (logits.float() - rl[:cut].float()).abs().max().item())
    print(f"continuous vs static, graph={graph}: max |logit difference| = {worst}")
    assert [len(t) for t, _ in out][:3] == LIMITS[:3] and len(out[3][0]) <= 18
    for i, (tokens, logits) in enumerate(out):
        assert torch.equal(logits, static_refs[graph, i][1][: len(tokens)]), i
    if not graph:  # the public entry point is the same loop
        pub = model.generate_continuous(LIMITS, input_tokens=PROMPTS, max_batch=3, page_size=PAGE, skinny_gemm=True,
                                        stop_tokens=[stop])
        for o, (tokens, logits) in zip(pub, out):
            assert o.completion_tokens == tokens and torch.equal(o.completion_logits, logits)


def test_sampled_admission_draws_once(model):
    s = Sampler(0.8, 40, 0.95, seed=3)
    dec = model.continuous_decoder(3, page_size=PAGE, max_pages=2, skinny_gemm=True, use_cuda_graph=True, sample_fn=s)
    assert s.step == 0  # the parked warm-up and capture passes burn no draws
    dec.admit(0, PROMPTS[0], 8)
    assert s.step == 1
    dec.step()
    dec.admit(2, PROMPTS[1], 8)
    assert s.step == 3
    dec.step()
    assert s.step == 4 and dec.captures == 1
    dec.state.check()


def _count(monkeypatch, names):
    calls: dict = {}
    mod = ext()
    for name in names:
        fn = getattr(mod, name)

        def wrapped(*a, _fn=fn, _name=name, **k):
            out = _fn(*a, **k)
            paged = _name == "fa_fwd" and ((len(a) > 16 and a[16] is not None) or k.get("block_table") is not None)
            key = _name + ("+table" if paged else "")
            calls[key] = calls.get(key, 0) + (out is not None)
            return out

        monkeypatch.setattr(mod, name, wrapped)
    return calls


def _taken(calls):
    return {k: v for k, v in calls.items() if v}


@pytest.mark.parametrize("kv_cache", [None, FP8])
def test_steps_take_the_paged_kernels(model, monkeypatch, kv_cache):
    dec = model.continuous_decoder(3, page_size=PAGE, max_pages=2, skinny_gemm=True, kv_cache=kv_cache)
    dec.admit(0, PROMPTS[0], 8)
    dec.admit(1, PROMPTS[3], 8)
    calls = _count(monkeypatch, ("rope_kv_append_paged", "rope_kv_append_batch", "rope_kv_append", "fa_fwd",
                                 "gemv_norm_rope"))
    for _ in range(4):
        dec.step()
    dec.state.check()
    assert _taken(calls) == {"rope_kv_append_paged": 4 * LAYERS, "fa_fwd+table": 4 * LAYERS}, calls
    sdec = model.batch_decoder(6, PROMPTS[:3], skinny_gemm=True, kv_cache=kv_cache, page_size=PAGE)
    calls.clear()  # the prefills ran the prefill kernels
    for _ in range(3):
        sdec.step()
    assert _taken(calls) == {"rope_kv_append_paged": 3 * LAYERS, "fa_fwd+table": 3 * LAYERS}, calls


def test_errors(model):
    with pytest.raises(ValueError, match="at most"):
        model.continuous_decoder(5, page_size=PAGE, max_pages=2, use_cuda_graph=True)
    with pytest.raises(ValueError, match="multiple of 32"):
        model.batch_decoder(4, PROMPTS[:2], page_size=48)
    dec = model.continuous_decoder(2, page_size=PAGE, max_pages=2, num_pages=2 + 2)
    with pytest.raises(ValueError, match="max_pages"):
        dec.admit(0, PROMPTS[0], 64)  # 7 + 64 > 2 * 32
    big = model.continuous_decoder(2, page_size=PAGE, max_pages=8)
    with pytest.raises(ValueError, match="sequence length"):
        big.admit(0, PROMPTS[0], 128)
    dec = model.continuous_decoder(2, page_size=PAGE, max_pages=2, num_pages=2 + 2)
    dec.admit(0, PROMPTS[2], 20)  # 33 tokens: two pages, the pool is empty
    before = (dec.state.pos.clone(), dec.state.block_table.clone(), dec.tok.clone())
    with pytest.raises(RuntimeError, match="4 pages"):
        dec.admit(1, PROMPTS[0], 4)
    assert dec.rows[1] is None and all(torch.equal(a, b) for a, b in
                                       zip(before, (dec.state.pos, dec.state.block_table, dec.tok)))
    dec.release(0)
    dec.admit(0, PROMPTS[0], 40)  # 7 tokens: one page; position 32 needs a second
    dec.admit(1, PROMPTS[1], 4)  # takes the last page
    for _ in range(25):
        dec.step()
    before = (dec.state.pos.clone(), dec.tok.clone())
    with pytest.raises(RuntimeError, match="4 pages"):
        dec.step()
    assert torch.equal(dec.state.pos, before[0]) and torch.equal(dec.tok, before[1]) and dec.rows[0].steps == 25
    with pytest.raises(RuntimeError, match="pages"):  # a static paged batch whose pool is too small, at construction
        model.batch_decoder(4, PROMPTS[:3], page_size=PAGE, num_pages=3 + 3)
