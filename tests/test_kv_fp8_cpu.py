"""FP8 e4m3 KV cache off the GPU: the row format (``ops.quant.quantize_kv_rows``), the cache classes, and
``generate_batch(kv_cache="fp8_e4m3")`` on the float32 CPU test model (K/V rounded to bf16, then quantised; attention is
the dense reference on the dequantised rows)."""
from types import SimpleNamespace

import pytest
import torch

from batch_decode_common import MAX_TOKENS, PROMPTS, make_model
from scaling_amd.core.nn.attention.attention import (BatchDecodeState, BatchStaticKVCache, BatchStaticKVCacheFP8,
                                                     DecodeState, KVCache, ParallelSelfAttention, StaticKVCacheFP8)
from scaling_amd.ops import quant
from scaling_amd.ops.attention import attention_reference, flash_attention
from scaling_amd.transformer.inference import batch_decode

FP8 = "fp8_e4m3"


def _from_codes(rows, nkv, hd, seed, exps=(-20, 20)):
    """A bf16 tensor [rows, nkv, hd] that IS an FP8 cache: random non-NaN codes, every row holding the code of 448 (so
    the row's scale is recoverable), times a power-of-two scale per row."""
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, 256, (rows, nkv, hd), generator=g, dtype=torch.int32)
    codes = torch.where((codes & 0x7F) == 0x7F, codes & 0x80, codes).to(torch.uint8)
    codes[..., 0] = 0x7E  # 448
    e = torch.randint(exps[0], exps[1] + 1, (nkv, rows), generator=g)
    scale = torch.ldexp(torch.ones(nkv, rows), e)
    x = codes.view(torch.float8_e4m3fn).float() * scale.t()[:, :, None]
    return x.to(torch.bfloat16), codes, scale


def test_quantize_kv_rows_round_trip_is_exact():
    x, codes, scale = _from_codes(37, 3, 64, 0)
    assert torch.equal(x.float(), codes.view(torch.float8_e4m3fn).float() * scale.t()[:, :, None])  # bf16 held it exactly
    q, s = quant.quantize_kv_rows(x)
    assert q.dtype == torch.uint8 and tuple(q.shape) == (37, 3, 64) and q.is_contiguous()
    assert s.dtype == torch.float32 and tuple(s.shape) == (3, 37) and s.is_contiguous()
    assert torch.equal(s, scale)
    # +0 / -0 are two codes of one value; everything else must come back as the same byte
    same = (q == codes) | (((q | codes) & 0x7F) == 0)
    assert bool(same.all())
    assert torch.equal(quant.dequantize_kv_rows(q, s), x)
    assert torch.equal(quant.dequantize_kv_rows(q.view(torch.float8_e4m3fn), s, torch.float32), x.float())


def test_quantize_kv_rows_is_quantize_rows_fp8_per_row():
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(9, 2, 32, generator=g) * torch.logspace(-30, 30, 9)[:, None, None]).to(torch.bfloat16)
    x[3, 1] = 0  # an all-zero row: scale 1
    q, s = quant.quantize_kv_rows(x)
    for r in range(9):
        for h in range(2):
            qr, sr = quant.quantize_rows_fp8(x[r, h].view(1, 32))
            assert torch.equal(qr.view(torch.uint8).view(-1), q[r, h]) and float(sr) == float(s[h, r])
    assert float(s[1, 3]) == 1.0 and not q[3, 1].any()
    with pytest.raises(ValueError, match="non-finite"):
        quant.quantize_kv_rows(torch.full((1, 1, 8), float("nan")))
    with pytest.raises(ValueError, match="rows, nkv, hd"):
        quant.quantize_kv_rows(torch.zeros(4, 8))
    with pytest.raises(ValueError, match="scales"):
        quant.dequantize_kv_rows(q, s.t().contiguous())


def test_static_cache_fp8_on_cpu():
    nkv, hd, n, cap = 2, 32, 5, 8
    g = torch.Generator().manual_seed(2)
    k, v = (torch.randn(n, nkv, hd, generator=g).to(torch.bfloat16) for _ in range(2))
    st = DecodeState(n, torch.device("cpu"))
    c = StaticKVCacheFP8.from_cache(KVCache.start(k, v), cap, st)
    assert c.k.dtype == c.v.dtype == torch.uint8 and tuple(c.k.shape) == (cap, nkv, hd)
    assert c.k_scale.dtype == torch.float32 and tuple(c.k_scale.shape) == tuple(c.v_scale.shape) == (nkv, cap)
    assert c.bytes_per_token() == 2 * nkv * (hd + 4)
    qk, sk = quant.quantize_kv_rows(k)
    assert torch.equal(c.k[:n], qk) and torch.equal(c.k_scale[:, :n], sk)
    assert not c.k[n:].any() and bool((c.k_scale[:, n:] == 1).all())
    k1, v1 = (torch.randn(1, nkv, hd, generator=g).to(torch.bfloat16) for _ in range(2))
    kc, vc, cu = c.append(k1, v1)
    assert kc is c.k and vc is c.v and cu is st.cu_k
    dk, dv = c.dequantized()
    assert dk.dtype == torch.bfloat16
    assert torch.equal(dk[n : n + 1], quant.dequantize_kv_rows(*quant.quantize_kv_rows(k1)))
    assert torch.equal(dv[n : n + 1], quant.dequantize_kv_rows(*quant.quantize_kv_rows(v1)))
    assert torch.equal(dk[:n], quant.dequantize_kv_rows(qk, sk)) and not dk[n + 1 :].any()
    st.check()
    # a non-finite value: no NaN code, the error word's second bit, and check() says so
    bad = k1.clone()
    bad[0, 0, 3], bad[0, 1, 5] = float("nan"), float("inf")
    st.advance()
    c.append(bad, v1)
    assert not bool(((c.k & 0x7F) == 0x7F).any()) and int(st.err) == 2
    row = c.dequantized()[0][n + 1]
    assert float(row[0, 3]) == 0.0 and float(row[1, 5]) == 2.0 ** 127 and float(c.k_scale[1, n + 1]) == 2.0 ** 119
    with pytest.raises(RuntimeError, match="NaN or above 2\\^127"):
        st.check()
    with pytest.raises(ValueError, match="bfloat16 models only"):
        StaticKVCacheFP8.from_cache(KVCache.start(k.half(), v.half()), cap, st)


def test_batch_cache_fp8_on_cpu():
    nkv, hd, cap = 2, 32, 6
    g = torch.Generator().manual_seed(3)
    lens = [2, 4, 1]
    kvs = [KVCache.start(*(torch.randn(n, nkv, hd, generator=g).to(torch.bfloat16) for _ in range(2))) for n in lens]
    st = BatchDecodeState(lens, cap, torch.device("cpu"))
    c = BatchStaticKVCacheFP8.from_caches(kvs, st)
    assert c.k.dtype == torch.uint8 and tuple(c.k.shape) == (3 * cap, nkv, hd) and tuple(c.k_scale.shape) == (nkv, 3 * cap)
    for b, (kv, n) in enumerate(zip(kvs, lens)):
        q, s = quant.quantize_kv_rows(kv.v[:n])
        assert torch.equal(c.v[b * cap : b * cap + n], q) and torch.equal(c.v_scale[:, b * cap : b * cap + n], s)
    k1, v1 = (torch.randn(3, nkv, hd, generator=g).to(torch.bfloat16) for _ in range(2))
    before = (c.k.clone(), c.k_scale.clone())
    st.pos[1] = cap  # outside its slab: nothing of sequence 1 may change, the error word is set
    c.append(k1, v1)
    assert int(st.err) == 1
    q, s = quant.quantize_kv_rows(k1)
    for b, n in enumerate(lens):
        if b == 1:
            assert torch.equal(c.k[cap : 2 * cap], before[0][cap : 2 * cap])
            assert torch.equal(c.k_scale[:, cap : 2 * cap], before[1][:, cap : 2 * cap])
        else:
            assert torch.equal(c.k[b * cap + n], q[b]) and torch.equal(c.k_scale[:, b * cap + n], s[:, b])
    with pytest.raises(RuntimeError, match="exceeded"):
        st.check()


def test_flash_attention_kv_scales_on_cpu():
    """CPU tensors: the dense reference on the dequantised rows, with either key form; the refusals."""
    x, codes, scale = _from_codes(40, 2, 32, 4, exps=(-3, 3))
    xv, vcodes, vscale = _from_codes(40, 2, 32, 5, exps=(-3, 3))
    g = torch.Generator().manual_seed(6)
    q = torch.randn(2, 4, 32, generator=g).to(torch.bfloat16)
    cu_q = torch.tensor([0, 1, 2], dtype=torch.int32)
    kr = torch.tensor([[0, 7], [20, 20]], dtype=torch.int32)
    with torch.no_grad():
        out = flash_attention(q, codes, vcodes, cu_q, max_seqlen_q=1, max_seqlen_k=20, key_ranges=kr,
                              kv_scales=(scale, vscale))
        ref = attention_reference(q, x, xv, cu_q, None, 32 ** -0.5, True, key_ranges=kr)
        assert torch.equal(out, ref)
        cu_k = torch.tensor([0, 7, 40], dtype=torch.int32)
        out = flash_attention(q, codes.view(torch.float8_e4m3fn), vcodes, cu_q, cu_k, 1, 33, kv_scales=(scale, vscale))
        assert torch.equal(out, attention_reference(q, x, xv, cu_q, cu_k, 32 ** -0.5, True))
        with pytest.raises(ValueError, match="bfloat16 queries"):
            flash_attention(q.half(), codes, vcodes, cu_q, cu_k, 1, 33, kv_scales=(scale, vscale))
        with pytest.raises(ValueError, match="kv heads, key rows"):
            flash_attention(q, codes, vcodes, cu_q, cu_k, 1, 33, kv_scales=(scale.t().contiguous(), vscale))
        with pytest.raises(ValueError, match="codes"):
            flash_attention(q, x, xv, cu_q, cu_k, 1, 33, kv_scales=(scale, vscale))
        with pytest.raises(ValueError, match="dropout"):
            flash_attention(q, codes, vcodes, cu_q, cu_k, 1, 33, dropout_p=0.1, training=True, kv_scales=(scale, vscale))


# ---------------------------------------------------------------------------------------------- generation
@pytest.fixture(scope="module")
def model():
    return make_model("cpu", "float32")


@pytest.fixture(scope="module")
def batch4(model):
    return model.generate_batch(MAX_TOKENS, input_tokens=PROMPTS[:4], stop_tokens=[], kv_cache=FP8)


def test_batched_equals_single_with_fp8_cache(model, batch4):
    for b in (0, 1, 2, 3):
        one = model.generate_batch(MAX_TOKENS, input_tokens=[PROMPTS[b]], stop_tokens=[], kv_cache=FP8)[0]
        assert one.completion_tokens == batch4[b].completion_tokens
        assert one.completion_logits.shape == (MAX_TOKENS, 256)
        # fp32 sum-order noise on O(1) logits is ~1e-6 (tests/test_batch_decode_cpu.py uses the same bound)
        torch.testing.assert_close(one.completion_logits, batch4[b].completion_logits, rtol=0, atol=1e-4)


def test_per_row_stop_tokens_with_fp8_cache(model, batch4):
    stops = [o.completion_tokens[5 + 6 * b] for b, o in enumerate(batch4)]
    outs = model.generate_batch(MAX_TOKENS, input_tokens=PROMPTS[:4], stop_tokens=stops, kv_cache=FP8)
    lengths = [len(o.completion_tokens) for o in outs]
    assert len(set(lengths)) > 1 and min(lengths) < MAX_TOKENS, lengths
    for o, full in zip(outs, batch4):
        n = len(o.completion_tokens)
        assert o.completion_tokens == full.completion_tokens[:n]
        assert o.completion_tokens[-1] in stops or n == MAX_TOKENS
        assert not any(t in stops for t in o.completion_tokens[:-1])
        assert torch.equal(o.completion_logits, full.completion_logits[:n])


class _DequantisedBatchCache(BatchStaticKVCache):
    """The oracle: a plain cache (the model's dtype) that holds what the FP8 cache encodes."""

    @staticmethod
    def _round(x):
        return quant.dequantize_kv_rows(*quant.quantize_kv_rows(x.to(torch.bfloat16)), dtype=x.dtype)

    @classmethod
    def from_caches(cls, kvs, state):
        for kv in kvs:
            kv.k[: kv.length] = cls._round(kv.k[: kv.length])
            kv.v[: kv.length] = cls._round(kv.v[: kv.length])
        c = BatchStaticKVCache.from_caches(kvs, state)
        return cls(c.k, c.v, state)

    def append(self, k, v):
        return super().append(self._round(k), self._round(v))


def test_fp8_cache_is_quantised_and_equals_the_dequantised_run(model, batch4, monkeypatch):
    plain = model.generate_batch(MAX_TOKENS, input_tokens=PROMPTS[:4], stop_tokens=[])
    # step 0 is the prefill (exact K/V); the later steps read quantised rows
    for p, f in zip(plain, batch4):
        assert torch.equal(p.completion_logits[0], f.completion_logits[0])
        assert not torch.equal(p.completion_logits[1], f.completion_logits[1])
    monkeypatch.setattr(batch_decode, "BatchStaticKVCache", _DequantisedBatchCache)
    oracle = model.generate_batch(MAX_TOKENS, input_tokens=PROMPTS[:4], stop_tokens=[])
    for o, f in zip(oracle, batch4):
        assert o.completion_tokens == f.completion_tokens
        assert torch.equal(o.completion_logits, f.completion_logits)


def test_cache_objects_of_a_decoder(model):
    dec = model.batch_decoder(4, PROMPTS[:2], kv_cache=FP8)
    assert dec.kv_cache == FP8
    for a in dec.attns:
        c = a.cache[0]
        assert isinstance(c, BatchStaticKVCacheFP8) and c.k.dtype == torch.uint8 and c.k.element_size() == 1
        assert tuple(c.k_scale.shape) == (c.k.shape[1], c.k.shape[0]) and c.k_scale.dtype == torch.float32
    assert model.batch_decoder(4, PROMPTS[:2]).kv_cache is None


def test_refusals(model):
    with pytest.raises(ValueError, match="unknown kv_cache scheme 'int8'"):
        model.generate_batch(4, input_tokens=PROMPTS[:2], stop_tokens=[], kv_cache="int8")
    with pytest.raises(ValueError, match="unknown kv_cache scheme"):
        model.batch_decoder(4, PROMPTS[:2], kv_cache="fp8")
    with pytest.raises(ValueError, match="unknown kv_cache scheme"):
        model.generate(4, input_tokens=PROMPTS[0], stop_tokens=[], use_cuda_graph=True, kv_cache="e5m2")
    with pytest.raises(ValueError, match="needs use_cuda_graph=True"):
        model.generate(4, input_tokens=PROMPTS[0], stop_tokens=[], kv_cache=FP8)
    with pytest.raises(ValueError, match="bfloat16 models only"):
        make_model("cpu", "float16").generate_batch(4, input_tokens=PROMPTS[:2], stop_tokens=[], kv_cache=FP8)
    with pytest.raises(ValueError, match="key_query_norm is not supported"):
        make_model("cpu", "float32", key_query_norm=True).generate_batch(4, input_tokens=PROMPTS[:2], stop_tokens=[],
                                                                         kv_cache=FP8)
    with pytest.raises(ValueError, match="non-flash"):
        make_model("cpu", "float32", masked_softmax={"kernel": "torch"}).generate_batch(
            4, input_tokens=PROMPTS[:2], stop_tokens=[], kv_cache=FP8)
    # tensor parallelism: a layer whose topology says model_parallel_size = 2 (as tests/test_quant_cpu.py does)
    tp = make_model("cpu", "float32")
    attn = [m for m in tp.modules() if isinstance(m, ParallelSelfAttention)]
    attn[1].topology = SimpleNamespace(config=SimpleNamespace(model_parallel_size=2))
    with pytest.raises(ValueError, match="tensor parallelism"):
        attn[1].check_fp8_kv_cache()
    attn[0].check_fp8_kv_cache()
    with pytest.raises(ValueError, match="tensor parallelism"):
        tp.generate_batch(4, input_tokens=PROMPTS[:2], stop_tokens=[], kv_cache=FP8)
    with pytest.raises(ValueError, match="tensor parallelism"):
        tp.batch_decoder(4, PROMPTS[:2], kv_cache=FP8)
    assert not any(a.cache for a in attn)  # refused before anything was prefilled
