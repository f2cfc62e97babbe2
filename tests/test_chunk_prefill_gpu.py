"""Chunked prefill into the paged KV cache on the GPU (``ContinuousBatchDecoder(prefill_chunk=...)``): prefill and
teacher-forced decode logits against the unchunked decoder, the FP8-KV error against the unchunked FP8-KV admit's own,
the kernel taken, one capture, serving.  The small model of ``tests/batch_decode_common.py`` with a 256-token rotary
table; the 150-token prompt goes in as chunks of 64, 64 and 22 with a 32-token page boundary inside each."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from batch_decode_common import PROMPTS, make_model  # noqa: E402
from scaling_amd.ops._ext import ext  # noqa: E402

LAYERS = 2
FP8 = "fp8_e4m3"
BOUND = 5e-2  # tests/test_batch_decode_skinny_gpu.py's bound for logits of different kernel paths on this model
PROMPT = torch.randint(1, 256, (150,), generator=torch.Generator().manual_seed(0)).tolist()  # 0 would start a sequence


@pytest.fixture(scope="module")
def model():
    return make_model(0, "bfloat16", sequence_length=256)


@pytest.fixture(scope="module")
def twin():
    return make_model(0, "bfloat16", sequence_length=256)  # the same weights: a model holds one decoder's pools at a time


def _decoder(model, chunk, graph=False, kv_cache=None):
    return model.continuous_decoder(3, page_size=32, max_pages=5, skinny_gemm=True, use_cuda_graph=graph,
                                    kv_cache=kv_cache, prefill_chunk=chunk)


@pytest.mark.parametrize("graph", [False, True])
def test_chunked_admit_and_teacher_forced_steps(model, twin, monkeypatch, graph):
    ref, dec = _decoder(twin, None, graph), _decoder(model, 64, graph)
    calls = []
    fa_chunk = ext().fa_chunk
    monkeypatch.setattr(ext(), "fa_chunk", lambda *a, **k: calls.append(a[0].shape[0]) or fa_chunk(*a, **k))
    r0, r1 = ref.admit(1, PROMPT, 9), dec.admit(1, PROMPT, 9)
    assert calls == [64] * LAYERS + [64] * LAYERS + [22] * LAYERS, calls  # the chunk passes took the new kernel
    assert all(dec.spare_index not in a.cache and list(a.cache) == [0] for a in dec.attns)
    diff = (r0.logits[0].float() - r1.logits[0].float()).abs().max().item()
    print(f"prefill logits: max abs diff {diff:.3e}")
    assert diff <= BOUND
    for step in range(8):
        dec.tok.copy_(ref.tok)  # teacher forcing: both feed the reference's tokens
        ref.step()
        dec.step()
        diff = (ref.rec_logits[step, 1].float() - dec.rec_logits[step, 1].float()).abs().max().item()
        print(f"step {step}: max abs diff {diff:.3e}")
        assert diff <= BOUND, step
    dec.state.check()
    assert dec.captures == (1 if graph else 0) and len(calls) == 3 * LAYERS  # no recapture; decode steps: decode kernel


def test_fp8_kv_error_is_of_the_unchunked_admit_s_size(model):
    """Relative RMS difference of the prefill logits to their bf16-KV counterparts: the chunked FP8-KV admit's (prompt
    keys quantised before the prompt's own later chunks read them) is at most twice the unchunked path's own difference
    between FP8-KV and bf16-KV admits of the same prompt -- measured here on existing code, not on the code under test."""
    def rel_rms(a, b):
        return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()

    # the unchunked admit prefills against exact bf16 K/V whatever the cache: its prefill logits carry no FP8 error, so
    # its FP8 error shows in the first decode step, which reads the quantised prompt
    def logits(chunk, kv_cache):  # (prefill, first decode step)
        dec = _decoder(model, chunk, kv_cache=kv_cache)
        first = dec.admit(1, PROMPT, 8).logits[0].float()
        dec.step()
        dec.state.check()
        return first, dec.rec_logits[0, 1].float()

    parent = rel_rms(logits(None, FP8)[1], logits(None, None)[1])
    (p8, s8), (p16, s16) = logits(64, FP8), logits(64, None)
    prefill, step = rel_rms(p8, p16), rel_rms(s8, s16)
    print(f"relative RMS difference FP8-KV vs bf16-KV: unchunked first step {parent:.3e}, chunked prefill "
          f"{prefill:.3e}, chunked first step {step:.3e}")
    assert 0 < prefill <= 2 * parent


def test_serve_and_errors(model):
    requests = [(PROMPTS[i], n) for i, n in ((2, 5), (0, 9), (5, 3), (3, 7))]
    kw = dict(page_size=32, max_pages=3, skinny_gemm=True)
    ref = model.continuous_decoder(2, **kw).serve(requests, [])
    got = model.continuous_decoder(2, prefill_chunk=32, **kw).serve(requests, [])
    assert [len(t) for t, _ in got] == [len(t) for t, _ in ref] == [n for _, n in requests]
    assert all(torch.isfinite(lg).all() for _, lg in got)
    with pytest.raises(ValueError, match="multiple of 32"):
        model.continuous_decoder(2, prefill_chunk=48, **kw)
