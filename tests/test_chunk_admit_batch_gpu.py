"""Batched chunked admission on the GPU (``ContinuousBatchDecoder.admit_many``): prompts of 150, 33, 64 and 97 tokens
with ``prefill_chunk=64`` -- they end in passes 2, 0, 0 and 1, one exactly on a chunk edge -- against four single admits
on a twin decoder, and the exhausted pool.  The small model of ``tests/batch_decode_common.py``, 256 rotary rows."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from batch_decode_common import make_model  # noqa: E402
from scaling_amd.core.nn.attention.attention import PagedKVCache, PagedKVCacheFP8  # noqa: E402
from scaling_amd.ops._ext import ext  # noqa: E402

LAYERS = 2
BOUND = 5e-2  # tests/test_chunk_prefill_gpu.py's bound: different row counts may pick different library GEMM algorithms
PROMPTS = [torch.randint(1, 256, (n,), generator=torch.Generator().manual_seed(n)).tolist() for n in (150, 33, 64, 97)]


@pytest.fixture(scope="module")
def models():
    return make_model(0, "bfloat16", sequence_length=256), make_model(0, "bfloat16", sequence_length=256)


def _decoder(model, graph=False, kv_cache=None, num_pages=None):
    return model.continuous_decoder(4, page_size=32, max_pages=5, num_pages=num_pages, skinny_gemm=True,
                                    use_cuda_graph=graph, kv_cache=kv_cache, prefill_chunk=64)


@pytest.mark.parametrize("kv_cache", [None, "fp8_e4m3"])
@pytest.mark.parametrize("graph", [False, True])
def test_admit_many_against_single_admits(models, monkeypatch, graph, kv_cache):
    ref, dec = _decoder(models[1], graph, kv_cache), _decoder(models[0], graph, kv_cache)
    r0 = [ref.admit(b, p, 9) for b, p in enumerate(PROMPTS)]
    fused, unfused = [], []
    kernel = ext().rope_kv_write_chunk
    monkeypatch.setattr(ext(), "rope_kv_write_chunk", lambda *a, **k: fused.append(a[0].shape[0]) or kernel(*a, **k))
    for cls in (PagedKVCache, PagedKVCacheFP8):
        monkeypatch.setattr(cls, "write_rows", lambda *a, **k: unfused.append(1))
    r1 = dec.admit_many(range(4), PROMPTS, 9)
    # passes of 64 + 33 + 64 + 64, 64 + 33 and 22 tokens, each one fused launch per layer and no unfused write
    assert fused == [225] * LAYERS + [97] * LAYERS + [22] * LAYERS and not unfused
    for b in range(4):
        diff = (r0[b].logits[0].float() - r1[b].logits[0].float()).abs().max().item()
        print(f"prefill logits of prompt {b}: max abs diff {diff:.3e}")
        assert diff <= BOUND, b
    for step in range(8):
        dec.tok.copy_(ref.tok)  # teacher forcing
        ref.step()
        dec.step()
        diff = (ref.rec_logits[step].float() - dec.rec_logits[step].float()).abs().max().item()
        print(f"step {step}: max abs diff {diff:.3e}")
        assert diff <= BOUND, step
    dec.state.check()
    assert dec.captures == (1 if graph else 0)


def test_admit_many_with_a_pool_one_page_too_small_changes_nothing(models):
    dec = _decoder(models[0], num_pages=4 + 5 + 2 + 3 + 4 - 1)  # the parking pages and one less than the prompts' 14
    st = dec.state
    before = [list(dec.allocator._free), st.block_table.clone(), st.pos.clone()] + \
             [t.clone() for a in dec.attns for t in (a.cache[0].k, a.cache[0].v)]
    with pytest.raises(RuntimeError, match="pool holds 17 pages"):
        dec.admit_many(range(4), PROMPTS, 9)
    after = [list(dec.allocator._free), st.block_table, st.pos] + [t for a in dec.attns for t in (a.cache[0].k, a.cache[0].v)]
    assert before[0] == after[0] and all(torch.equal(x, y) for x, y in zip(before[1:], after[1:]))
    assert dec.free_rows == [0, 1, 2, 3]
