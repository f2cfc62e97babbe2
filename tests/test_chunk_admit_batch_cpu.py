"""Batched chunked admission off the GPU: ``generate_continuous(prefill_chunk=32)`` with five requests on three rows --
the first admission is one batch of three prompts, in two passes -- returns ``generate``'s greedy tokens per prompt."""
import torch

from batch_decode_common import make_model


def test_batched_admission_returns_generate_s_tokens(monkeypatch):
    model = make_model("cpu", "float32")
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(1, 256, (n,), generator=g).tolist() for n in (40, 7, 33, 64, 12)]
    batches = []
    from scaling_amd.transformer.inference.batch_decode import ContinuousBatchDecoder
    admit_many = ContinuousBatchDecoder.admit_many
    monkeypatch.setattr(ContinuousBatchDecoder, "admit_many",
                        lambda self, rows, *a, **k: batches.append(len(list(rows))) or admit_many(self, rows, *a, **k))
    got = model.generate_continuous(6, input_tokens=prompts, max_batch=3, page_size=32, stop_tokens=[], prefill_chunk=32)
    assert batches[0] == 3
    for p, o in zip(prompts, got):
        assert o.completion_tokens == model.generate(6, input_tokens=p, stop_tokens=[]).completion_tokens


def test_cpu_rope_kv_write_chunk_is_rotation_plus_write_rows():
    """The CPU path of ``ops.rope.rope_kv_write_chunk`` against ``apply_rope`` + ``write_rows`` per segment, bf16 and FP8
    pools, bytewise; a segment running past its pages sets bit 0, zeroes those q rows and writes nothing for them."""
    from scaling_amd.core.nn.attention.attention import PagedDecodeState, PagedKVCache, PagedKVCacheFP8
    from scaling_amd.ops.rope import apply_rope, rope_kv_write_chunk, rope_tables

    nq, nkv, hd, page = 4, 2, 16, 32
    cos, sin = rope_tables(hd, 128, 10000.0, True, torch.bfloat16, "cpu")
    x = torch.randn(50, nq + 2 * nkv, hd, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16)
    segs, pos = [([5, 2], 20, 30), ([7], 14, 20)], torch.cat([torch.arange(20, 50), torch.arange(14, 34)])
    table = torch.tensor([[5, 2], [7, -1]], dtype=torch.int32)
    for cls in (PagedKVCache, PagedKVCacheFP8):
        a, b = (cls.empty(nkv, hd, torch.bfloat16, PagedDecodeState(2, 2, page, 8, torch.device("cpu"))) for _ in range(2))
        q = rope_kv_write_chunk(x, cos, sin, torch.tensor([0, 30, 50], dtype=torch.int32), torch.tensor([20, 14]), table,
                                page, nq, nkv, hd, True, a.k, a.v, a.state.err, getattr(a, "scales", None))
        k = apply_rope(x[:, nq : nq + nkv], cos, sin, pos, hd, 1, True)
        b.write_rows(segs[0][0], 20, k[:30], x[:30, nq + nkv :])
        b.write_rows(segs[1][0], 14, k[30:48], x[30:48, nq + nkv :])  # positions 32, 33 lie past the one page
        assert torch.equal(q[:48], apply_rope(x[:48, :nq], cos, sin, pos[:48], hd, 1, True)) and (q[48:] == 0).all()
        assert a.state.err.item() == 1 and all(torch.equal(s, t) for s, t in zip((a.k, a.v) + tuple(getattr(a, "scales", ())),
                                                                              (b.k, b.v) + tuple(getattr(b, "scales", ()))))
