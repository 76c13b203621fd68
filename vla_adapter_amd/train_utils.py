"""Mirror of prismatic/training/train_utils.py:8-58 (the two action masks, token accuracy, decoded-action L1).  On CUDA int64 labels the union the hot
path consumes comes from the native ``vla_action_mask`` kernel (see engine.VLAEngine.forward); these functions keep
the reference's names/semantics for logging code that wants the two masks separately (index arithmetic only).  The token-CE
trainer does not call the two metric functions either: ``vla_token_ce_metrics`` counts the same quantities inside the loss kernel
(trainers.BackboneTrainer.token_metrics); they are the reference's API on tensors, for evaluation code and the tests."""
import torch

from .constants import ACTION_DIM, ACTION_TOKEN_BEGIN_IDX, IGNORE_INDEX


def get_current_action_mask(token_ids: torch.Tensor) -> torch.Tensor:
    cumsum = torch.cumsum(token_ids != IGNORE_INDEX, dim=1)
    return ((1 <= cumsum) & (cumsum <= ACTION_DIM)) & (token_ids > ACTION_TOKEN_BEGIN_IDX)


def get_next_actions_mask(token_ids: torch.Tensor) -> torch.Tensor:
    cumsum = torch.cumsum(token_ids != IGNORE_INDEX, dim=1)
    return (cumsum > ACTION_DIM) & (token_ids > ACTION_TOKEN_BEGIN_IDX)


def compute_token_accuracy(predicted_token_ids: torch.Tensor, ground_truth_token_ids: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """train_utils.py:44-47: correct predictions under the mask / mask size, one f32 division (0 / 0 = NaN for an empty mask)."""
    correct_preds = (predicted_token_ids == ground_truth_token_ids) & mask
    return correct_preds.sum().float() / mask.sum().float()


def compute_actions_l1_loss(action_tokenizer, predicted_token_ids: torch.Tensor, ground_truth_token_ids: torch.Tensor,
                            mask: torch.Tensor) -> torch.Tensor:
    """train_utils.py:50-58: mean |centre(pred) - centre(truth)| over the masked positions.  ``action_tokenizer``: anything with the
    reference's ``decode_token_ids_to_actions`` - input_stage.GPUInputStage decodes tensors where they live (no numpy round trip).
    An empty mask gives NaN, as the reference's l1_loss of two empty tensors does."""
    dec = action_tokenizer.decode_token_ids_to_actions
    pred, true = torch.as_tensor(dec(predicted_token_ids[mask])), torch.as_tensor(dec(ground_truth_token_ids[mask]))
    return torch.nn.functional.l1_loss(pred, true)


def all_actions_positions(labels: torch.Tensor, shift: int = 0):
    """Native path: (qidx, pos, count) of the union mask on labels[:, shift:] (int32 device tensors, no host sync)."""
    from . import ops
    return ops.action_mask(labels.contiguous(), shift)
