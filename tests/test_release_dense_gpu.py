"""``quantize_weights(scheme, release_dense=True)`` on the small model of ``tests/batch_decode_common.py`` (256-token
rotary table): the memory released, the quantised-weight GEMM taken by prefills above the decode row limit, logits
against the twin that keeps its bf16 weights (same seed, same scheme), one composition case and the refusals."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from batch_decode_common import PROMPTS, make_model  # noqa: E402
from scaling_amd.ops import gemm, quant  # noqa: E402
from test_batch_decode_skinny_gpu import LAYERS, _count  # noqa: E402

BOUND = 5e-2  # tests/test_chunk_prefill_gpu.py's bound between two prefill paths that differ in summation order
PROMPT = torch.randint(1, 256, (150,), generator=torch.Generator().manual_seed(0)).tolist()
GROUPS = 4 * LAYERS  # q/k/v, the o-projection, gate/up, down


@pytest.fixture(scope="module", params=quant.SCHEMES)
def trio(request):
    """(scheme, the dense-kept module, the released module, its summary, bytes of the module before / after)."""
    kept = make_model(0, "bfloat16", sequence_length=256)
    kept.quantize_weights(request.param)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    rel = make_model(0, "bfloat16", sequence_length=256)
    dense = torch.cuda.memory_allocated() - base
    info = rel.quantize_weights(request.param, release_dense=True)
    torch.cuda.synchronize()
    return request.param, kept, rel, info, dense, torch.cuda.memory_allocated() - base


def test_memory_is_released(trio):
    _, kept, rel, info, dense, after = trio
    assert info["skipped"] == {} and info["tensors"] == 3 * LAYERS + 4 * LAYERS
    assert info["released_bytes"] == info["bf16_bytes"] > 0
    # 512 bytes of allocator rounding per tensor involved: every freed weight, and per group the codes, scales and stub
    slack = 512 * (info["tensors"] + 3 * GROUPS)
    want = dense - info["bf16_bytes"] + info["quantized_bytes"]
    print(f"dense {dense} B, released {after} B, expected {want} B +- {slack}")
    assert abs(after - want) <= slack
    released = [n for n, p in rel.named_parameters() if quant.released_name(p) is not None]
    assert len(released) == info["tensors"]
    assert [(n, p.shape, p.dtype, p.device) for n, p in rel.named_parameters()] == \
           [(n, p.shape, p.dtype, p.device) for n, p in kept.named_parameters()]


def test_prefill_takes_qgemm_and_agrees(trio, monkeypatch):
    scheme, kept, rel, _, _, _ = trio
    name = "qgemm_w8" if scheme == quant.SCHEME else "qgemm_w4"
    calls = _count(monkeypatch, ("qgemm_w8", "qgemm_w4"))
    for n in (70, 150):
        got = rel.logits(input_tokens=PROMPT[:n]).float()
        assert calls == {name: GROUPS}, calls  # every linear layer but the tied, never-quantised head
        calls.clear()
        diff = (got - kept.logits(input_tokens=PROMPT[:n]).float()).abs().max().item()
        assert calls == {}, calls  # the dense-kept twin prefills from its bf16 weights
        print(f"{scheme}, {n} tokens: max |logit difference| {diff:.3e}")
        assert diff <= BOUND, n


def test_graph_decode_steps_agree(trio):
    scheme, kept, rel, _, _, _ = trio
    ref, dec = kept.batch_decoder(9, [PROMPT[:70]]), rel.batch_decoder(9, [PROMPT[:70]])
    ref.capture()
    dec.capture()
    for _ in range(8):
        dec.tok.copy_(ref.tok)  # teacher forcing: both feed the reference's tokens
        ref.step()
        dec.step()
    dec.state.check()
    diff = (dec.logits[:9].float() - ref.logits[:9].float()).abs().amax(dim=(1, 2))
    print(f"{scheme}: max |logit difference| per step:", [round(float(d), 4) for d in diff])
    assert float(diff.max()) <= BOUND


@pytest.mark.parametrize("trio", [quant.SCHEME_MXFP4], indirect=True)  # one composition case: the MXFP4 module
def test_continuous_chunked_prefill_composes(trio):
    _, kept, rel, _, _, _ = trio
    kw = dict(input_tokens=[PROMPT[:100], PROMPTS[2], PROMPTS[0]], max_batch=2, prefill_chunk=64, page_size=64,
              skinny_gemm=True, stop_tokens=[])
    want, got = kept.generate_continuous([5, 7, 4], **kw), rel.generate_continuous([5, 7, 4], **kw)
    assert [len(o.completion_tokens) for o in got] == [len(o.completion_tokens) for o in want] == [5, 7, 4]
    for g, w in zip(got, want):
        assert (g.completion_logits[0].float() - w.completion_logits[0].float()).abs().max().item() <= BOUND


def test_refusals(trio, tmp_path):
    scheme, _, rel, _, _, _ = trio
    with pytest.raises(RuntimeError, match="released"):
        rel.quantize_weights(scheme)
    with pytest.raises(RuntimeError, match="released"):
        rel.state_dict()
    with pytest.raises(RuntimeError, match="released"):
        rel.save_checkpoint(tmp_path)
    w = next(p for p in rel.parameters() if quant.released_name(p) is not None)
    x = torch.zeros(80, w.shape[1], dtype=w.dtype, device=w.device, requires_grad=True)
    with torch.enable_grad(), pytest.raises(RuntimeError, match="released"):
        gemm.linear(x, w)
    with pytest.raises(RuntimeError, match="released"):
        rel.train()
