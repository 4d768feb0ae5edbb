"""Batch inference over the GPUs of one node: bucketed prompt batches (prompts.py) and the utterance-sharded sampler + gather (sharded.py); the validation loss of a checkpoint and the duration loss of a duration predictor, forward only (validate.py); the pruning workbench: distillation losses of a (teacher, student) pair and the block ablation scan (distill.py), block selection and checkpoint surgery (prune.py); speaker similarity of generated audio against its prompt, the ECAPA-TDNN head of the reference's SIM figure (speaker.py) and the WavLM feature extractor in front of it (wavlm.py)."""
from .distill import DistillLoss, block_ablation, distillation_loss, subset_losses  # noqa: F401
from .prune import prune_checkpoint, prune_state_dict, select_blocks  # noqa: F401
from .prompts import get_inference_prompt, infer_prompts, padded_mel_batch, ragged_sample_fn, sample_kwargs, synthetic_metainfo  # noqa: F401
from .speaker import SpeakerEncoder, speaker_similarity, wrapper_similarity  # noqa: F401
from .wavlm import WavLMExtractor  # noqa: F401
from .sharded import gather_utterances, sample_sharded, split_between_processes  # noqa: F401
from .validate import DurationLoss, ValidationLoss, duration_validation_loss, validation_loss  # noqa: F401
