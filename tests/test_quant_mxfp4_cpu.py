"""MXFP4 weight-only quantisation (``scaling_amd/ops/quant.py``, scheme ``"mxfp4"``) on CPU: the quantiser's properties,
group copies, stale copies and ``TransformerInferenceModule.quantize_weights("mxfp4")``.

The copy is an exact encoding of the bf16 parameter it replaces (e2m1 codes times power-of-two block scales), so every
check here is bitwise or a property of the format itself.

Idempotence.  Quantising the dequantised matrix returns the same VALUES bit for bit, and the same codes and scales in
every block whose maximum did not round down to the code of 3.  The exception follows from the scale rule itself, as
for FP8 (``test_quant_cpu.py``): a block with ``amax / s`` in ``(3, 3.5)`` dequantises to ``amax' = 3 s``, for which
``s' = 2^ceil(log2(3 s / 6)) = s / 2`` and every code doubles -- the same bf16 values, encoded once more from then on
(the second re-quantisation repeats codes and scales everywhere).
"""
from __future__ import annotations

import warnings
from types import SimpleNamespace

import pytest
import torch

from scaling_amd.ops import quant
from scaling_amd.ops.gemm import linear
from scaling_amd.ops.quant import dequantize_rows_mxfp4, quantize_rows_mxfp4

N_ROWS = 24
GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def make_weight(K: int, seed: int = 0, n: int = N_ROWS) -> torch.Tensor:
    """Seeded bf16 [n, K]: N(0,1)/sqrt(K) rows scaled by 2^(i % 12 - 6); row 1 all zero; row 2 with a zero first block
    only; row 4 with one element 2^14 x the row's maximum (its block's other codes are zero); row 5 tiny (2^-110:
    the scale exponent is clamped)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, K, generator=g) / K ** 0.5
    w = w * torch.tensor([2.0 ** (i % 12 - 6) for i in range(n)])[:, None]
    w[1] = 0
    w[2, :32] = 0
    w[4, K // 5] = 2.0 ** 14 * w[4].abs().max()
    w[5] = w[5] * 2.0 ** -110
    return w.bfloat16()


def _scale_values(scales: torch.Tensor) -> torch.Tensor:
    return torch.ldexp(torch.ones(()), scales.to(torch.int32) - 127)


def _nibbles(codes: torch.Tensor) -> torch.Tensor:
    """[N, K] code values 0..15 in k order from the packed bytes: even k in the low nibble."""
    return torch.stack([codes & 15, codes >> 4], dim=2).reshape(codes.shape[0], -1)


@pytest.mark.parametrize("K", [32, 64, 4096])
def test_quantiser_properties(K):
    w = make_weight(K)
    codes, scales = quantize_rows_mxfp4(w)
    assert codes.shape == (N_ROWS, K // 2) and codes.dtype == torch.uint8
    assert scales.shape == (N_ROWS, K // 32) and scales.dtype == torch.uint8
    s = _scale_values(scales)
    amax = w.float().view(N_ROWS, -1, 32).abs().amax(dim=2)
    zero = amax == 0
    assert zero[1].all() and zero[2, 0]
    assert (scales[zero] == 127).all()  # s = 1 for all-zero blocks
    clamped = scales.int() - 127 == quant._MIN_EXP
    assert clamped[5].all() or K == 32  # (row 5 is far below the clamp)
    r = (amax / s)[~zero & ~clamped]
    assert (r > 3).all() and (r <= 6).all()
    assert (amax / s <= 6)[clamped].all()
    assert int(scales.max()) < 255
    nib = _nibbles(codes)
    assert not (nib == 8).any()  # no -0
    # exact in bf16 and fp32, and equal to the brute-force nearest grid point of w / s (ties: see test_tie_midpoints)
    d32 = dequantize_rows_mxfp4(codes, scales, torch.float32)
    d16 = dequantize_rows_mxfp4(codes, scales, torch.bfloat16)
    assert d16.dtype == torch.bfloat16 and torch.equal(d16.float(), d32)
    a = (w.float().view(N_ROWS, -1, 32) / s[:, :, None]).abs().reshape(N_ROWS, K).double()
    err = (a - GRID.double()[(nib & 7).long()]).abs()
    best = (a[:, :, None] - GRID.double()[None, None, :]).abs().amin(dim=2)
    assert torch.equal(err, best)
    neg = (nib >> 3).bool()
    assert torch.equal(neg, (w.float() < 0) & ((nib & 7) > 0))
    # relative error: half a grid step of at most 2 on a block maximum above 3
    blk_err = (d32 - w.float()).abs().view(N_ROWS, -1, 32).amax(dim=2)
    assert (blk_err <= s)[~clamped].all()
    # idempotence (module docstring)
    c2, s2 = quantize_rows_mxfp4(d16)
    assert torch.equal(dequantize_rows_mxfp4(c2, s2, torch.bfloat16).view(torch.int16), d16.view(torch.int16))
    top = _nibbles(codes).view(N_ROWS, -1, 32).bitwise_and(7).amax(dim=2)  # the block's largest code index
    # index 5 is the code of 3; a block under the exponent clamp may hold zero codes only and re-quantises as a zero block
    same = (top != 5) & ((top != 0) | zero)
    assert (top != 0)[~zero & ~clamped].all()
    assert torch.equal(scales[same], s2[same])
    assert torch.equal(codes.view(N_ROWS, -1, 16)[same], c2.view(N_ROWS, -1, 16)[same])
    assert (s2.int() == scales.int() - 1)[(top == 5) & ~clamped].all()
    c3, s3 = quantize_rows_mxfp4(dequantize_rows_mxfp4(c2, s2, torch.bfloat16))
    assert torch.equal(c3, c2) and torch.equal(s3, s2)


def test_tie_midpoints_round_to_the_even_code():
    mids = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    want = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    for sc in (1.0, 2.0 ** -9, 2.0 ** 7):
        row = torch.zeros(64)
        row[:7] = torch.tensor(mids) * sc
        row[7] = 6.0 * sc  # pins the block scale to sc
        row[32:39] = -torch.tensor(mids) * sc
        row[39] = -6.0 * sc
        codes, scales = quantize_rows_mxfp4(row.bfloat16()[None])
        assert torch.equal(_scale_values(scales), torch.tensor([[sc, sc]]))
        d = dequantize_rows_mxfp4(codes, scales, torch.float32)[0]
        assert d[:8].tolist() == [v * sc for v in want] + [6.0 * sc]
        assert d[32:40].tolist() == [-v * sc for v in want] + [-6.0 * sc]
        assert (d[:1] == 0).all() and not torch.signbit(d[32]).item()  # -0.25 -> +0: no -0 code
        assert not (_nibbles(codes) == 8).any()


def test_nibble_order_and_every_code():
    # weight 2i in the low nibble, weight 2i + 1 in the high nibble
    vals = torch.cat([GRID, -GRID[1:], torch.zeros(17)])  # 8 + 7 + 17 = 32
    codes, scales = quantize_rows_mxfp4(vals.bfloat16()[None])
    assert scales.tolist() == [[127]]
    want = list(range(8)) + [9, 10, 11, 12, 13, 14, 15] + [0] * 17
    assert _nibbles(codes)[0].tolist() == want
    assert codes[0, 0].item() == (1 << 4) | 0 and codes[0, 4].item() == (10 << 4) | 9
    # the decoder takes every byte, a hand-placed -0 included, and e8m0 scales
    allc = torch.arange(16, dtype=torch.uint8).repeat(2)[None]  # 32 codes -> 16 bytes
    packed = (allc[:, 0::2] | (allc[:, 1::2] << 4))
    d = dequantize_rows_mxfp4(packed, torch.tensor([[130]], dtype=torch.uint8), torch.float32)[0]
    assert d[:16].tolist() == [v * 8 for v in GRID.tolist()] + [-v * 8 for v in GRID.tolist()]
    assert d[8].item() == 0.0
    if hasattr(torch, "float4_e2m1fn_x2"):  # the same packing as torch's dtype (bytes only: it has no arithmetic)
        assert packed.view(torch.float4_e2m1fn_x2).view(torch.uint8).equal(packed)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf"), 2.0 ** 121, -(2.0 ** 125)])
def test_quantiser_refusals(bad):
    w = make_weight(64)
    w[7, 9] = bad
    with pytest.raises(ValueError):
        quantize_rows_mxfp4(w)


def test_quantiser_shape_refusals_and_limit():
    with pytest.raises(ValueError, match="32"):
        quantize_rows_mxfp4(torch.zeros(4, 48).bfloat16())
    with pytest.raises(ValueError):
        quantize_rows_mxfp4(torch.zeros(64).bfloat16())
    w = make_weight(64)
    w[7, 9] = 2.0 ** 120  # the limit itself is taken
    codes, scales = quantize_rows_mxfp4(w)
    assert torch.isfinite(dequantize_rows_mxfp4(codes, scales)).all()


def test_stale_copy_is_dropped():
    w = torch.nn.Parameter(make_weight(64), requires_grad=False)
    quant.quantize_parameters([w], "mxfp4")
    assert not hasattr(w, "_sa_w8") and quant.w8_of(w) is None
    c, s = quant.w4_of(w)
    assert quant.wq_of(w)[0] == "_w4"
    assert torch.equal(w.data, dequantize_rows_mxfp4(c, s, torch.bfloat16))
    x = torch.randn(2, 64, generator=torch.Generator().manual_seed(1)).bfloat16()
    assert torch.equal(linear(x, w), torch.nn.functional.linear(x, w))
    assert quant.w4_of(w) is not None
    w.add_(1)
    quant._warned[0] = False
    with pytest.warns(RuntimeWarning, match="MXFP4 copy"):
        y = linear(x, w)
    assert not hasattr(w, "_sa_w4") and quant.wq_of(w) is None
    assert torch.equal(y, torch.nn.functional.linear(x, w))
    with warnings.catch_warnings():  # dropped once: nothing left to warn about
        warnings.simplefilter("error")
        linear(x, w)


def test_group_copies_are_slices_of_one_buffer():
    from scaling_amd.core.nn.linear.main_grad import adjacent_w8, adjacent_wq

    ws = [torch.nn.Parameter(make_weight(64, seed=i, n=n), requires_grad=False) for i, n in enumerate((16, 8, 8))]
    before = torch.cat([w.data for w in ws])
    b16, bq = quant.quantize_parameters(ws, "mxfp4")
    assert (b16, bq) == (32 * 64 * 2, 32 * 32 + 32 * 2)
    sfx, c, s = adjacent_wq(ws)
    assert sfx == "_w4" and c.shape == (32, 32) and s.shape == (32, 2) and adjacent_w8(ws) is None
    cc, ss = quantize_rows_mxfp4(before)
    assert torch.equal(c, cc) and torch.equal(s, ss)
    assert quant.w4_of(ws[1])[0].data_ptr() == c.data_ptr() + 16 * 32
    assert quant.w4_of(ws[1])[1].data_ptr() == s.data_ptr() + 16 * 2
    # re-quantising in the other scheme replaces the copies, and back
    quant.quantize_parameters(ws)
    assert adjacent_wq(ws)[0] == "_w8" and not any(hasattr(w, "_sa_w4") for w in ws)
    quant.quantize_parameters(ws, "mxfp4")
    assert adjacent_wq(ws)[0] == "_w4" and not any(hasattr(w, "_sa_w8") for w in ws)
    ws[2].mul_(2)
    quant._warned[0] = True
    assert adjacent_wq(ws) is None and quant.w4_of(ws[0]) is not None
    with pytest.raises(ValueError, match="scheme"):
        quant.quantize_parameters(ws, "int4")


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
    info = m.quantize_weights("mxfp4")
    assert info["scheme"] == "mxfp4" and info["tensors"] == 2 * 7 and info["skipped"] == {}
    assert info["fp8_bytes"] == 0 and info["quantized_bytes"] * 64 == info["bf16_bytes"] * 17  # 0.53125 B / weight
    quantised = {n for n, p in m.named_parameters() if hasattr(p, "_sa_w4")}
    assert len(quantised) == 14 and all(".self_attention." in n or ".mlp." in n for n in quantised)
    assert not any(hasattr(p, "_sa_w8") for p in m.parameters())
    changed = 0
    for n, p in m.named_parameters():
        if n in quantised:  # the masters equal the dequantised values
            c, s = quant.w4_of(p)
            assert torch.equal(p.data, dequantize_rows_mxfp4(c, s, torch.bfloat16)), n
            changed += int(not torch.equal(p.data, original[n]))
        else:  # embedding, norms, head: untouched
            assert torch.equal(p.data, original[n]), n
    assert changed == 14
    # a second call changes no value bitwise
    snap = {n: p.detach().clone() for n, p in m.named_parameters()}
    m.quantize_weights("mxfp4")
    for n, p in m.named_parameters():
        assert torch.equal(p.data.view(torch.int16), snap[n].view(torch.int16)), n
    # greedy cached generation equals a never-quantised twin that was handed the same values
    twin = _module()
    with torch.no_grad():
        for (n, p), (n2, p2) in zip(m.named_parameters(), twin.named_parameters()):
            assert n == n2
            p2.copy_(p)
    assert not any(quant.has_copy(p) for p in twin.parameters())
    prompt = [3, 17, 42, 99, 5, 7, 11]
    a = m.generate(10, input_tokens=prompt, stop_tokens=[], use_cache=True)
    b = twin.generate(10, input_tokens=prompt, stop_tokens=[], use_cache=True)
    assert a.completion_tokens == b.completion_tokens and len(a.completion_tokens) == 10
    assert torch.equal(a.completion_logits, b.completion_logits)
    assert all(quant.w4_of(p) is not None for n, p in m.named_parameters() if n in quantised)


def test_switching_schemes_requantises_and_drops_the_old_copies():
    m = _module(weight_tying=False)
    m.quantize_weights("fp8_e4m3", include_lm_head=True)
    head = m._layers[-1].linear.weight
    assert hasattr(head, "_sa_w8")
    info = m.quantize_weights("mxfp4")
    assert info["tensors"] == 14 and not any(hasattr(p, "_sa_w8") for p in m.parameters())
    assert not quant.has_copy(head)
    for p in m.parameters():
        if hasattr(p, "_sa_w4"):
            c, s = quant.w4_of(p)
            assert torch.equal(p.data, dequantize_rows_mxfp4(c, s))
    info = m.quantize_weights("fp8_e4m3")
    assert info["fp8_bytes"] == info["quantized_bytes"] > 0
    assert not any(hasattr(p, "_sa_w4") for p in m.parameters())
    assert sum(hasattr(p, "_sa_w8") for p in m.parameters()) == 14


def test_quantize_weights_lm_head_and_skips():
    m = _module(weight_tying=False)
    assert m.quantize_weights("mxfp4")["tensors"] == 14 and not hasattr(m._layers[-1].linear.weight, "_sa_w4")
    info = m.quantize_weights("mxfp4", include_lm_head=True)
    assert info["tensors"] == 15 and hasattr(m._layers[-1].linear.weight, "_sa_w4")
    tied = _module(weight_tying=True)
    info = tied.quantize_weights("mxfp4", include_lm_head=True)
    assert info["tensors"] == 14 and list(info["skipped"].values()) == ["tied to the embedding"]
    # hidden 144 / 4 heads: q/k/v/dense/gate/up have K = 144 (a multiple of 16, not of 32), down has K = 288
    odd = _module(hidden_size=144, num_attention_heads=4, attention_num_kv_heads=2)
    info = odd.quantize_weights("mxfp4")
    assert info["tensors"] == 2 and len(info["skipped"]) == 12
    assert all("multiple of 32" in r for r in info["skipped"].values())
    assert all(n.endswith("mlp.dense_out.weight") for n, p in odd.named_parameters() if hasattr(p, "_sa_w4"))
    assert odd.quantize_weights("fp8_e4m3")["tensors"] == 14  # the FP8 scheme takes K = 144


def test_quantize_weights_rejects_unsupported():
    with pytest.raises(ValueError, match="scheme"):
        _module().quantize_weights("int4")
    with pytest.raises(RuntimeError, match="bfloat16"):
        _module(precision="float32").quantize_weights("mxfp4")
    with pytest.raises(RuntimeError, match="one device"):
        _module(devices=("cpu", "cpu")).quantize_weights("mxfp4")
    m = _module()
    m._layers[1].topology = SimpleNamespace(config=SimpleNamespace(model_parallel_size=2))
    with pytest.raises(RuntimeError, match="tensor parallelism"):
        m.quantize_weights("mxfp4")
    lora = _module(lora_config={"name": "lora", "rank": 4, "parallel_modules": ["query", "value"]})
    with pytest.raises(RuntimeError, match="LoRA"):
        lora.quantize_weights("mxfp4")
    assert not any(quant.has_copy(p) for p in lora.parameters())
