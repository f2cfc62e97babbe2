from .batch_decode import BatchDecoder, ContinuousBatchDecoder
from .inference_model import CompletionOutput, TransformerInferenceModule
from .sample import Sampler, fast_multinomial, sample_argmax, sample_temperature, top_k_transform, top_p_transform

__all__ = [
    "BatchDecoder",
    "CompletionOutput",
    "ContinuousBatchDecoder",
    "Sampler",
    "TransformerInferenceModule",
    "fast_multinomial",
    "sample_argmax",
    "sample_temperature",
    "top_k_transform",
    "top_p_transform",
]
