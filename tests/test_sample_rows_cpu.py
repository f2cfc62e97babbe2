"""Per-request sampling off the GPU: the float64 twin of the row-table sampler (``ops.sample.sample_rows`` on CPU
tensors) and ``generate_continuous(..., sampling=...)`` through it, on the float32 model of ``batch_decode_common``."""
import pytest
import torch

from batch_decode_common import PROMPTS, make_model
from scaling_amd.ops.sample import sample_rows
from scaling_amd.transformer.inference import RequestSampler, Sampler, SamplingParams

SP = SamplingParams


@pytest.fixture(scope="module")
def model():
    return make_model("cpu", "float32")


def test_twin_semantics():
    rs = RequestSampler(4, 3)
    rs.set_row(0, SP(temperature=0.0, repetition_penalty=2.0), [1, 7])  # 7 >= V is ignored
    rs.set_row(1, SP(temperature=0.0, presence_penalty=1.5, penalize_prompt=False), [1])
    rs.set_row(2, SP(temperature=0.0, repetition_penalty=2.0), [1, 1, 1])  # full history
    x = torch.tensor([[0.5, 3.0, 2.0, -1.0]]).repeat(4, 1)
    before = rs.table.buf.clone()
    tokens, info = sample_rows(x, rs.table, want_info=torch.full((4, 2), -7, dtype=torch.int32))
    # rows 0, 2: 3.0 / 2 = 1.5 < 2.0; row 1: the prompt is not history; row 3 is parked
    assert tokens.tolist() == [2, 1, 2, 0]
    assert info[:3, 0].tolist() == [1, 1, 1] and info[:3, 1].view(torch.float32).tolist() == [2.0, 3.0, 2.0]
    assert info[3].tolist() == [-7, -7] and torch.equal(rs.table.buf[3], before[3])
    assert rs.table.hist_len.tolist() == [3, 1, 3, 0] and rs.table.step.tolist() == [1, 1, 1, 0]
    assert rs.table.hist[0].tolist() == [1, 7, 2] and rs.table.hist[1, 0].item() == 1
    assert torch.equal(rs.table.hist[2], before[2, 12:15])  # nothing appended at hist_len == H
    # call 2 penalises what call 1 drew: row 0 sees {1, 2} (1.5 > 1.0), row 1 now sees token 1 (3.0 - 1.5 < 2.0)
    assert sample_rows(x, rs.table).tolist() == [1, 2, 2, 0]
    wrong = rs.table.rows(0, 4)
    wrong.step = wrong.top_k
    with pytest.raises(ValueError, match="column step"):
        sample_rows(x, wrong)
    for bad in (SP(temperature=-1.0), SP(repetition_penalty=0.0), SP(top_p=float("nan"))):
        with pytest.raises(ValueError):
            rs.set_row(3, bad)


def test_generate_continuous_per_request(model):
    params = [SP(0.9, 40, 0.95, seed=1), SP(0.9, 40, 0.95, seed=2), SP(0.9, 40, 0.95, seed=1),
              SP(0.0), SP(1.0, seed=5, repetition_penalty=1.3, presence_penalty=0.5)]
    prompts = [PROMPTS[0], PROMPTS[0], PROMPTS[0], PROMPTS[3], PROMPTS[4]]
    outs = model.generate_continuous(12, input_tokens=prompts, max_batch=2, page_size=32, stop_tokens=[], sampling=params)
    toks = [o.completion_tokens for o in outs]
    assert all(len(t) == 12 for t in toks)
    assert toks[0] == toks[2] and toks[0] != toks[1]  # the seed, not the row or the admission time, decides
    greedy = model.generate_continuous(12, input_tokens=[PROMPTS[3]], max_batch=2, page_size=32, stop_tokens=[])
    assert toks[3] == greedy[0].completion_tokens
    # every request replayed alone on its recorded logits, in row 0 of a fresh table: the same tokens
    for p, prompt, o in zip(params, prompts, outs):
        rs = RequestSampler(1, 64)
        rs.set_row(0, p, prompt)
        again = [int(rs(lg[None, None])) for lg in o.completion_logits]
        assert again == o.completion_tokens, p
        assert rs.table.hist[0, : len(prompt) + 12].tolist() == list(prompt) + again


def test_errors_before_anything_is_allocated(model, monkeypatch):
    from scaling_amd.transformer.inference import batch_decode

    def no_alloc(*a, **k):
        raise AssertionError("allocated")

    monkeypatch.setattr(batch_decode, "PageAllocator", no_alloc)
    rs = RequestSampler(2, 64)
    with pytest.raises(ValueError, match="RequestSampler"):
        model.generate(4, input_tokens=PROMPTS[0], stop_tokens=[], sample_fn=rs)
    with pytest.raises(ValueError, match="RequestSampler"):
        model.generate_batch(4, input_tokens=PROMPTS[:2], stop_tokens=[], sample_fn=rs)
    with pytest.raises(ValueError, match="sample_fn"):
        model.generate_continuous(4, input_tokens=PROMPTS[:2], stop_tokens=[], sample_fn=Sampler(), sampling=SP())
    with pytest.raises(ValueError, match="sample_fn"):
        model.continuous_decoder(2, page_size=32, sample_fn=Sampler(), sampling=True)
    with pytest.raises(ValueError, match="temperature"):
        model.generate_continuous(4, input_tokens=PROMPTS[:2], stop_tokens=[], sampling=SP(temperature=-0.5))
    for wrong in ([SP()], True, [SP(), 0.7]):
        with pytest.raises(ValueError, match="one per request"):
            model.generate_continuous(4, input_tokens=PROMPTS[:2], stop_tokens=[], sampling=wrong)
    monkeypatch.undo()
    dec = model.continuous_decoder(2, page_size=32)
    with pytest.raises(ValueError, match="RequestSampler"):
        dec.admit(0, PROMPTS[0], 4, sampling=SP())
    assert dec.allocator.in_use == 0
    # an admission that fails after the sampler's row was filled parks that row again
    dec = model.continuous_decoder(2, page_size=32, sampling=True)

    def boom(*a, **k):
        raise RuntimeError("assign")

    monkeypatch.setattr(dec.state, "assign", boom)
    with pytest.raises(RuntimeError, match="assign"):
        dec.admit(0, PROMPTS[0], 4, sampling=SP())
    assert not bool(dec.sample_fn.table.active.any()) and dec.rows[0] is None
