"""AtMan score manipulation as a per-key bias, on the CPU: the embedding's zero-stride tensor, the dense path computing
the same from it, the flash layer's routing (the CPU ``chunk_attention`` is the dense reference) and ``key_bias`` itself."""
import math

import pytest
import torch

from atman_common import CONTROLS, PROMPT, prompt_logits, twins
from scaling_amd.ops.attention import chunk_attention
from scaling_amd.transformer.model.layers import EmbeddingInput


@pytest.fixture(scope="module")
def models():
    return twins("cpu", "float32")


@pytest.mark.parametrize("log_additive", [True, False])
def test_embedding_view_and_dense_path(models, monkeypatch, log_additive):
    seen, build, s = [], EmbeddingInput._attention_manipulation, len(PROMPT)
    monkeypatch.setattr(EmbeddingInput, "_attention_manipulation", lambda *a: seen.append(build(*a)) or seen[-1])
    got = prompt_logits(models[1], CONTROLS["two_mixed"], log_additive)
    old = torch.full((1, 1, s, s), 0.0 if log_additive else 1.0)  # the materialised construction
    for j, f in CONTROLS["two_mixed"]:
        old[0, :, :, j] = f if not log_additive else (-10000.0 if f == 0.0 else float(torch.log(torch.tensor(f))))
    assert seen[0].shape == old.shape and seen[0].dtype == old.dtype and seen[0].stride(2) == 0
    assert torch.equal(seen[0].contiguous(), old)
    monkeypatch.setattr(EmbeddingInput, "_attention_manipulation", lambda *a: build(*a).contiguous())
    assert torch.equal(got, prompt_logits(models[1], CONTROLS["two_mixed"], log_additive))  # same bits from a copy


@pytest.mark.parametrize("cached", [False, True])
@pytest.mark.parametrize("log_additive", [True, False])
def test_flash_layer_honours_the_controls(models, log_additive, cached):
    got = prompt_logits(models[0], CONTROLS["two_mixed"], log_additive, cached)
    torch.testing.assert_close(got, prompt_logits(models[1], CONTROLS["two_mixed"], log_additive, cached), atol=1e-4, rtol=1e-4)
    assert (got - prompt_logits(models[0], cached=cached)).abs().max() > 1e-2  # fp32 both; the controls move far more


def test_cpu_chunk_attention_adds_the_bias_by_buffer_row():
    g = torch.Generator().manual_seed(1)
    q, k, v = torch.randn(5, 4, 32, generator=g), torch.randn(20, 2, 32, generator=g), torch.randn(20, 2, 32, generator=g)
    bias = torch.zeros(20)
    bias[9], bias[11], bias[12] = math.log(0.3), -10000.0, float("-inf")
    cu, kr = torch.tensor([0, 5], dtype=torch.int32), torch.tensor([[7, 9]], dtype=torch.int32)  # keys: rows 7..15
    s = torch.einsum("qhd,khd->hqk", q, k[7:16].repeat_interleave(2, 1)) / math.sqrt(32) + bias[7:16]
    s = s.masked_fill(torch.arange(9)[None, :] > torch.arange(5)[:, None] + 4, float("-inf"))
    ref = torch.einsum("hqk,khd->qhd", torch.softmax(s, -1), v[7:16].repeat_interleave(2, 1))
    torch.testing.assert_close(chunk_attention(q, k, v, cu, kr, 5, 9, key_bias=bias), ref, atol=1e-5, rtol=1e-5)
