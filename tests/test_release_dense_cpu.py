"""``quantize_weights(..., release_dense=...)`` on a CPU module: releasing is refused (the CPU path computes from the
bf16 parameters), and without it the summary is today's plus ``released_bytes == 0``."""
import pytest
from batch_decode_common import make_model

from scaling_amd.ops import quant


@pytest.mark.parametrize("scheme", quant.SCHEMES)
def test_release_dense_on_cpu(scheme):
    m = make_model("cpu", "bfloat16")
    with pytest.raises(ValueError, match="release_dense"):
        m.quantize_weights(scheme, release_dense=True)
    assert not any(quant.has_copy(p) for p in m.parameters())  # refused before anything was quantised
    info = m.quantize_weights(scheme, release_dense=False)
    assert set(info) == {"scheme", "tensors", "bf16_bytes", "fp8_bytes", "quantized_bytes", "skipped", "released_bytes"}
    assert info["released_bytes"] == 0 and info["tensors"] == 14
    assert all(quant.released_name(p) is None for p in m.parameters())
