"""Shared by tests/test_atman_flash_{cpu,gpu}.py: the small model of tests/batch_decode_common.py as a flash / torch pair
with equal weights and one pass over a 70-token prompt (two 64-key tiles) under AtMan controls."""
import torch

from batch_decode_common import make_model

PROMPT = torch.randint(1, 256, (70,), generator=torch.Generator().manual_seed(0)).tolist()  # 0 would start a sequence
# (token index, factor); never token 0: the dense path masks with -10000, so a row whose only visible key is suppressed
# with factor 0 is the one row on which it and a flash kernel (masked = -inf) are not the same function
CONTROLS = {"one_zero": [(37, 0.0)], "two_mixed": [(5, 0.3), (66, 0.0)]}


def twins(device, precision):
    return [make_model(device, precision, masked_softmax={"kernel": k}) for k in ("flash_attention", "torch")]


def prompt_logits(model, controls=None, log_additive=True, cached=False):
    """fp32 logits [s, vocab]; ``cached``: the pass that starts a KV cache (use_cache, reset_cache)."""
    from scaling_amd.transformer.data.inference_settings import Control, InferenceSettings, InferenceSuppressionParameters
    from scaling_amd.transformer.data.text_dataset_batch import TextDatasetBatch

    params = controls and [InferenceSuppressionParameters(None, log_additive, [Control(token_index=j, factor=f) for j, f in controls])]
    st = InferenceSettings(cached, cached, 0, [-1], inference_control_parameters=params)
    return model.forward(TextDatasetBatch(input_token_ids=torch.tensor([PROMPT]), inference_settings=st)).activations[0].float()
