"""Shared by tests/test_batch_decode_cpu.py and tests/test_batch_decode_gpu.py: the small Llama-layout model of
tests/test_decode_fp8_gpu.py and the fixed prompts (lengths 7, 1, 33, 12, then 9 and 20 for B = 6).

With max_tokens = 36 the 1-token row crosses the 32-key tile boundary, the 33-token row crosses 64, and the rows sit
at different positions in every step."""
import torch

MAX_TOKENS = 36
PROMPTS = [
    [3, 17, 42, 99, 5, 7, 11],
    [200],
    [17, 204, 38, 73, 56, 91, 226, 201, 167, 50, 155, 232, 156, 225, 172, 230, 166, 175, 21, 30, 82, 180, 22, 32, 28,
     144, 213, 85, 110, 66, 166, 152, 20],
    [184, 203, 229, 114, 232, 18, 231, 241, 195, 96, 219, 94],
    [89, 221, 172, 112, 228, 231, 96, 230, 252],
    [57, 121, 5, 217, 197, 174, 58, 142, 144, 32, 185, 100, 165, 161, 97, 164, 77, 63, 200, 69],
]
assert [len(p) for p in PROMPTS] == [7, 1, 33, 12, 9, 20]


def make_model(device, precision, **kw):
    from scaling_amd.transformer.context.config import TransformerArchitectureConfig
    from scaling_amd.transformer.inference import TransformerInferenceModule
    from scaling_amd.transformer.model.model import get_transformer_layer_specs

    cfg = dict(vocab_size=256, hidden_size=256, num_layers=2, num_attention_heads=4, sequence_length=128,
               norm_type="rms", mlp_type="swiglu", mlp_factor=2.0, precision=precision, attention_num_kv_heads=2,
               attention_qkv_in_one=False, relative_position_embedding_type="rotary_complex",
               masked_softmax={"kernel": "flash_attention"}, attention_bias=False, mlp_bias=False)
    cfg.update(kw)
    torch.manual_seed(0)
    return TransformerInferenceModule(get_transformer_layer_specs(TransformerArchitectureConfig(**cfg)), devices=(device,))
