"""FP8 weight-only quantisation (``scaling_amd/ops/quant.py``) on CPU: the quantiser's properties, stale copies and
``TransformerInferenceModule.quantize_weights``.

The FP8 copy is an exact encoding of the bf16 parameter it replaces (power-of-two row scales), so every check here is
bitwise or a property of the e4m3 format itself; there is no "quantisation error" tolerance.
"""
from __future__ import annotations

import warnings
from types import SimpleNamespace

import pytest
import torch

from scaling_amd.ops import quant
from scaling_amd.ops.gemm import linear
from scaling_amd.ops.quant import dequantize_rows_fp8, quantize_rows_fp8

N_ROWS = 48


def make_weight(K: int, seed: int = 0, n: int = N_ROWS) -> torch.Tensor:
    """Seeded bf16 [n, K]: N(0,1)/sqrt(K) rows scaled by 2^(i % 12 - 6); row 1 all zero; row 2 with one element 40x
    the row's maximum; row 4 with one element 2^14 x the row's maximum, so that most of its codes are subnormal or
    zero; row 3 with its maximum at 225/256 of a power of two, so that it rounds DOWN to the code 224."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, K, generator=g) / K ** 0.5
    w = w * torch.tensor([2.0 ** (i % 12 - 6) for i in range(n)])[:, None]
    w[1] = 0
    w[2, K // 3] = 40 * w[2].abs().max()
    w[4, K // 5] = 2.0 ** 14 * w[4].abs().max()
    w[3] = w[3].clamp(-0.4, 0.4)
    w[3, 5] = -225.0 / 256
    return w.bfloat16()


def _codes() -> torch.Tensor:
    """The 127 finite non-negative e4m3fn values, indexed by code 0x00..0x7E."""
    return torch.arange(127, dtype=torch.uint8).view(torch.float8_e4m3fn).float()


def _brute_force(v: torch.Tensor) -> torch.Tensor:
    """Nearest finite e4m3fn code of every element of fp32 ``v`` (ties to the even code, the sign kept), as bytes."""
    mag = _codes().double()
    d = (v.abs().double().reshape(-1, 1) - mag[None, :]).abs()
    best = d.min(dim=1, keepdim=True).values
    cand = d == best  # one code, or two neighbours on a tie
    idx = torch.arange(127)[None, :].expand_as(cand)
    lo = torch.where(cand, idx, torch.full_like(idx, 1000)).min(dim=1).values
    hi = torch.where(cand, idx, torch.full_like(idx, -1)).max(dim=1).values
    pick = torch.where(lo % 2 == 0, lo, hi).to(torch.uint8)
    sign = (torch.signbit(v).reshape(-1).to(torch.uint8)) << 7
    return (pick | sign).reshape(v.shape)


@pytest.mark.parametrize("K", [64, 512, 4096])
def test_quantiser_properties(K):
    w = make_weight(K)
    q, s = quantize_rows_fp8(w)
    assert q.shape == w.shape and q.element_size() == 1 and s.shape == (w.shape[0],) and s.dtype == torch.float32
    amax = w.float().abs().amax(dim=1)
    # exact powers of two; amax / s in (224, 448] for non-zero rows, s = 1 for the zero row
    m, _ = torch.frexp(s)
    assert bool((m == 0.5).all())
    assert s[1].item() == 1.0 and amax[1].item() == 0.0
    nz = amax > 0
    ratio = amax[nz] / s[nz]
    assert bool((ratio > 224).all()) and bool((ratio <= 448).all()), (ratio.min().item(), ratio.max().item())
    # no NaN code
    qb = q.view(torch.uint8)
    assert not bool(((qb & 0x7F) == 0x7F).any())
    # the cast equals the brute-force nearest-code search with ties to the even code
    v = w.float() / s[:, None]
    assert torch.equal(qb, _brute_force(v))
    sub = (v[4].abs() < 2.0 ** -6).float().mean().item()
    assert sub > 0.5 and bool(((qb[4] & 0x78) == 0).any() and ((qb[4] & 0x7F) != 0).any()), sub  # exponent-0 codes
    # dequantisation is bit-exact in bf16: no rounding of q * s
    d = dequantize_rows_fp8(q, s, torch.bfloat16)
    assert d.dtype == torch.bfloat16 and torch.equal(d.float(), q.float() * s[:, None])
    # relative error of normal-range values
    normal = v.abs() >= 2.0 ** -6
    rel = ((d.float() - w.float()).abs() / w.float().abs().clamp_min(1e-30))[normal]
    assert rel.max().item() <= 2.0 ** -4
    # quantise-of-dequantise: bitwise idempotent.  One case follows from the scale rule itself: a row whose maximum
    # rounded DOWN to the code 224 (amax / s in (224, 232], row 3 here) dequantises to amax' = 224 s, for which
    # s' = 2^ceil(log2(224 s / 448)) = s / 2 and every code doubles -- the same bf16 values, encoded once more
    # from then on.  Everywhere else (q, s) repeat bit for bit.
    q2, s2 = quantize_rows_fp8(d)
    d2 = dequantize_rows_fp8(q2, s2, torch.bfloat16)
    assert torch.equal(d2.view(torch.int16), d.view(torch.int16))
    halved = nz.clone()
    halved[nz] = q.float().abs().amax(dim=1)[nz] == 224
    assert bool(halved[3])
    keep = ~halved
    assert torch.equal(s2[keep], s[keep]) and torch.equal(q2.view(torch.uint8)[keep], qb[keep])
    assert torch.equal(s2[halved], s[halved] / 2) and torch.equal(q2.float()[halved], 2 * q.float()[halved])
    q3, s3 = quantize_rows_fp8(d2)
    assert torch.equal(s3, s2) and torch.equal(q3.view(torch.uint8), q2.view(torch.uint8))


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_quantiser_refuses_non_finite(bad):
    w = make_weight(64)
    w[7, 9] = bad
    with pytest.raises(ValueError):
        quantize_rows_fp8(w)


def test_stale_copy_is_dropped():
    w = torch.nn.Parameter(make_weight(64), requires_grad=False)
    quant.quantize_parameters([w])
    q, s = quant.w8_of(w)
    assert torch.equal(w.data, dequantize_rows_fp8(q, s, torch.bfloat16))
    x = torch.randn(2, 64, generator=torch.Generator().manual_seed(1)).bfloat16()
    assert torch.equal(linear(x, w), torch.nn.functional.linear(x, w))
    assert quant.w8_of(w) is not None
    w.add_(1)
    quant._warned[0] = False
    with pytest.warns(RuntimeWarning, match="FP8 copy"):
        y = linear(x, w)
    assert not hasattr(w, "_sa_w8") and quant.w8_of(w) is None
    assert torch.equal(y, torch.nn.functional.linear(x, w))
    with warnings.catch_warnings():  # dropped once: nothing left to warn about
        warnings.simplefilter("error")
        linear(x, w)


def test_group_copies_are_slices_of_one_buffer():
    from scaling_amd.core.nn.linear.main_grad import adjacent_w8

    ws = [torch.nn.Parameter(make_weight(64, seed=i, n=n), requires_grad=False) for i, n in enumerate((16, 8, 8))]
    before = torch.cat([w.data for w in ws])
    quant.quantize_parameters(ws)
    q, s = adjacent_w8(ws)
    assert q.shape == (32, 64) and s.shape == (32,)
    qq, ss = quantize_rows_fp8(before)
    assert torch.equal(q.view(torch.uint8), qq.view(torch.uint8)) and torch.equal(s, ss)
    assert quant.w8_of(ws[1])[0].data_ptr() == q.data_ptr() + 16 * 64
    ws[2].mul_(2)
    quant._warned[0] = True
    assert adjacent_w8(ws) is None and quant.w8_of(ws[0]) is not None


def _arch(**kw):
    from scaling_amd.transformer.context.config import TransformerArchitectureConfig

    base = dict(vocab_size=256, hidden_size=256, num_layers=2, num_attention_heads=4, sequence_length=128,
                norm_type="rms", mlp_type="swiglu", mlp_factor=2.0, precision="bfloat16", attention_num_kv_heads=2,
                attention_qkv_in_one=False, relative_position_embedding_type="rotary_complex",
                masked_softmax={"kernel": "torch"}, attention_bias=False, mlp_bias=False)
    base.update(kw)
    return TransformerArchitectureConfig(**base)


def _module(devices=("cpu",), **kw):
    from scaling_amd.transformer.inference import TransformerInferenceModule
    from scaling_amd.transformer.model.model import get_transformer_layer_specs

    torch.manual_seed(0)
    return TransformerInferenceModule(get_transformer_layer_specs(_arch(**kw)), devices=devices)


def test_quantize_weights_cpu_module():
    m = _module()
    original = {n: p.detach().clone() for n, p in m.named_parameters()}
    info = m.quantize_weights()
    assert info["tensors"] == 2 * 7 and info["skipped"] == {}
    assert info["fp8_bytes"] * 2 == info["bf16_bytes"] + 8 * sum(p.shape[0] for p in m.parameters() if hasattr(p, "_sa_w8"))
    quantised = {n for n, p in m.named_parameters() if hasattr(p, "_sa_w8")}
    assert len(quantised) == 14 and all(".self_attention." in n or ".mlp." in n for n in quantised)
    changed = 0
    for n, p in m.named_parameters():
        if n in quantised:  # the masters equal the dequantised values
            q, s = quant.w8_of(p)
            assert torch.equal(p.data, dequantize_rows_fp8(q, s, torch.bfloat16)), n
            changed += int(not torch.equal(p.data, original[n]))
        else:  # embedding, norms, head: untouched
            assert torch.equal(p.data, original[n]), n
    assert changed == 14
    # a second call changes nothing bitwise
    snap = {n: p.detach().clone() for n, p in m.named_parameters()}
    codes = {n: tuple(t.clone() for t in quant.w8_of(p)) for n, p in m.named_parameters() if n in quantised}
    m.quantize_weights()
    for n, p in m.named_parameters():
        assert torch.equal(p.data.view(torch.int16), snap[n].view(torch.int16)), n
        if n in quantised:
            q, s = quant.w8_of(p)
            assert torch.equal(dequantize_rows_fp8(q, s), dequantize_rows_fp8(*codes[n])), n
    # greedy cached generation equals a never-quantised twin that was handed the same values
    twin = _module()
    with torch.no_grad():
        for (n, p), (n2, p2) in zip(m.named_parameters(), twin.named_parameters()):
            assert n == n2
            p2.copy_(p)
    assert not any(hasattr(p, "_sa_w8") for p in twin.parameters())
    prompt = [3, 17, 42, 99, 5, 7, 11]
    a = m.generate(10, input_tokens=prompt, stop_tokens=[], use_cache=True)
    b = twin.generate(10, input_tokens=prompt, stop_tokens=[], use_cache=True)
    assert a.completion_tokens == b.completion_tokens and len(a.completion_tokens) == 10
    assert torch.equal(a.completion_logits, b.completion_logits)
    assert all(quant.w8_of(p) is not None for n, p in m.named_parameters() if n in quantised)


def test_quantize_weights_lm_head_and_skips():
    m = _module(weight_tying=False)
    assert m.quantize_weights()["tensors"] == 14 and not hasattr(m._layers[-1].linear.weight, "_sa_w8")
    info = m.quantize_weights(include_lm_head=True)
    assert info["tensors"] == 15 and hasattr(m._layers[-1].linear.weight, "_sa_w8")
    tied = _module(weight_tying=True)
    info = tied.quantize_weights(include_lm_head=True)
    assert info["tensors"] == 14 and list(info["skipped"].values()) == ["tied to the embedding"]
    # hidden 136 / 4 heads: q/k/v/dense/gate/up have K = 136 (not a multiple of 16), down has K = 272
    odd = _module(hidden_size=136, num_attention_heads=4, attention_num_kv_heads=2)
    info = odd.quantize_weights()
    assert info["tensors"] == 2 and len(info["skipped"]) == 12
    assert all("multiple of 16" in r for r in info["skipped"].values())
    assert all(n.endswith("mlp.dense_out.weight") for n, p in odd.named_parameters() if hasattr(p, "_sa_w8"))


def test_quantize_weights_rejects_unsupported():
    with pytest.raises(ValueError, match="scheme"):
        _module().quantize_weights("int4")
    with pytest.raises(RuntimeError, match="bfloat16"):
        _module(precision="float32").quantize_weights()
    with pytest.raises(RuntimeError, match="one device"):
        _module(devices=("cpu", "cpu")).quantize_weights()
    m = _module()
    m._layers[1].topology = SimpleNamespace(config=SimpleNamespace(model_parallel_size=2))
    with pytest.raises(RuntimeError, match="tensor parallelism"):
        m.quantize_weights()
    lora = _module(lora_config={"name": "lora", "rank": 4, "parallel_modules": ["query", "value"]})
    with pytest.raises(RuntimeError, match="LoRA"):
        lora.quantize_weights()
    assert not any(hasattr(p, "_sa_w8") for p in lora.parameters())
