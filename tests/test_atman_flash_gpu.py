"""AtMan controls on the flash path on the GPU: a flash model against its torch-kernel twin (bf16, equal weights).  The
bound is measured: the twins' logit difference WITHOUT controls is the existing kernels' disagreement; under controls
twice that is allowed (the manipulated scores go through the same two roundings)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from atman_common import CONTROLS, prompt_logits, twins  # noqa: E402
from scaling_amd.ops._ext import ext  # noqa: E402


@pytest.fixture(scope="module")
def models():
    flash, dense = twins(0, "bfloat16")
    return flash, dense, (prompt_logits(flash) - prompt_logits(dense)).abs().max().item()


@pytest.mark.parametrize("cached", [False, True])
@pytest.mark.parametrize("case,log_additive", [("one_zero", True), ("two_mixed", True), ("two_mixed", False)])
def test_controls_match_the_torch_twin_and_take_effect(models, monkeypatch, case, log_additive, cached):
    flash, dense, base = models
    plain, calls, fa_chunk = prompt_logits(flash, cached=cached), [], ext().fa_chunk
    monkeypatch.setattr(ext(), "fa_chunk", lambda *a, **k: calls.append(a[-1] is not None) or fa_chunk(*a, **k))
    got = prompt_logits(flash, CONTROLS[case], log_additive, cached)
    # every layer's attention: the chunk kernel with a key bias; multiplicative mode: the dense branch, nothing dropped
    assert calls == ([True, True] if log_additive else []), calls
    diff = (got - prompt_logits(dense, CONTROLS[case], log_additive, cached)).abs().max().item()
    moved = (got - plain).abs().max().item()
    print(f"{case} {log_additive} {cached}: flash vs torch {diff:.3e} (without controls {base:.3e}); controls move {moved:.3e}")
    assert base > 0 and diff <= 2 * base
    assert moved > 2 * base  # the controls take effect: they were dropped before
    if cached:  # the pass filled the cache as an unmanipulated pass does
        assert [m.self_attention.cache[0].length for m in flash.modules() if hasattr(m, "self_attention")] == [len(got)] * 2
