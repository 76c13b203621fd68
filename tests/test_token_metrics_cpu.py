"""The reference's token-CE training metrics as API twins on tensors (prismatic/training/train_utils.py:44-58,
prismatic/vla/action_tokenizer.py:76-95) against tests/golden/token_metrics.npz, which tools/make_golden_token_metrics.py recorded
from the reference's own functions.  No GPU: the twins are index arithmetic."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "token_metrics.npz")
RTOL = 1e-6          # the reference averages in fp64 (numpy bin centres) / divides in f32; ours is the same arithmetic or one f32 division


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def stage(gold):
    from vla_adapter_amd.input_stage import GPUInputStage
    return GPUInputStage("cpu", tokenizer_len=int(gold["tokenizer_len"]), n_bins=int(gold["n_bins"]))


def close(got: float, want: float) -> bool:
    return (got != got) if want != want else abs(got - want) <= RTOL * abs(want)


def test_fixture_holds_the_cases_it_was_made_for(gold):
    pred, gt = gold["pred_ids"], gold["gt_ids"]
    assert pred.shape == gt.shape == (3, 95)
    act = gt > 151386
    assert {0, 151386, 151643, 151935} <= set(pred[act].tolist()), "predicted ids outside the action range"
    assert {151387, 151642} <= set(gt[act].tolist()) and {151387, 151642} <= set(pred[act].tolist()), "the two extreme bins"
    assert (gt == -100).any(axis=1).all() and len({int((r == -100).argmin()) for r in gt}) == 3, "ragged prompts, IGNORE padding"
    assert gold["mask_counts"].tolist() == [[17, 116], [6, 58], [6, 58], [5, 0]]
    m = gold["metrics"]
    assert np.isnan(m).sum() == 2 and np.isnan(m[3, 2:]).all(), "NaN exactly where a sample has no next-actions row"


def test_masks_match_the_reference(gold):
    from vla_adapter_amd import train_utils as TU
    gt = torch.from_numpy(gold["gt_ids"])
    assert torch.equal(TU.get_current_action_mask(gt), torch.from_numpy(gold["current_mask"]))
    assert torch.equal(TU.get_next_actions_mask(gt), torch.from_numpy(gold["next_mask"]))


@pytest.mark.parametrize("case", range(4))
def test_twins_reproduce_the_reference_metrics(gold, stage, case):
    from vla_adapter_amd import train_utils as TU
    sl = [slice(0, 3), slice(0, 1), slice(1, 2), slice(2, 3)][case]
    pred, gt = torch.from_numpy(gold["pred_ids"])[sl], torch.from_numpy(gold["gt_ids"])[sl]
    cur, nxt = TU.get_current_action_mask(gt), TU.get_next_actions_mask(gt)
    got = [TU.compute_token_accuracy(pred, gt, cur), TU.compute_actions_l1_loss(stage, pred, gt, cur),
           TU.compute_token_accuracy(pred, gt, nxt), TU.compute_actions_l1_loss(stage, pred, gt, nxt)]
    for name, g, w in zip(("action_accuracy", "l1_loss", "next_actions_accuracy", "next_actions_l1_loss"), got, gold["metrics"][case]):
        assert g.dim() == 0
        print(f"{gold['cases'][case]} {name}: twin {float(g)!r}  reference {float(w)!r}")
        assert close(float(g), float(w)), (name, float(g), float(w))


def test_decode_matches_the_reference_bin_centres(gold, stage):
    """decode_token_ids_to_actions on every id of the vocabulary's action range and on the ids outside it that the fixture plants."""
    tl, nb = int(gold["tokenizer_len"]), int(gold["n_bins"])
    ids = torch.cat([torch.arange(tl - nb - 2, tl + 2), torch.tensor([0, 151935])])
    d = np.clip(tl - ids.numpy() - 1, 0, nb - 2)
    got = stage.decode_token_ids_to_actions(ids)
    assert got.dtype == torch.float64 and got.shape == ids.shape
    assert np.array_equal(got.numpy(), gold["bin_centers"][d])
    assert stage.decode_token_ids_to_actions(ids.view(2, -1)).shape == (2, ids.numel() // 2)


def test_bin_centres_are_equally_spaced(gold):
    """What lets the kernel sum integers: |centre[a] - centre[b]| = |a - b| * (max - min) / (n_bins - 1) to fp64 rounding."""
    c, nb = gold["bin_centers"], int(gold["n_bins"])
    a, b = np.meshgrid(np.arange(nb - 1), np.arange(nb - 1))
    assert np.abs(np.abs(c[a] - c[b]) - np.abs(a - b) * (2.0 / (nb - 1))).max() <= 4 * np.finfo(np.float64).eps


def test_decode_of_tokenize_is_the_identity_on_bin_indices(stage):
    """Tokenising a bin centre and decoding the id gives the same centre back, for every bin; the clipped ends (actions at or beyond
    +-1) land in the first / last bin.  tokenize on the CPU: np.digitize, what vla_action_tokenize implements on the device."""
    centres = stage.bin_centers.numpy()
    edges = stage.bins.numpy()

    def tokenize(a):
        return torch.from_numpy(stage.tokenizer_len - np.digitize(np.clip(a, stage.lo, stage.hi), edges))
    ids = tokenize(centres)
    assert np.array_equal(stage.tokenizer_len - ids.numpy() - 1, np.arange(centres.size)), "bin k is token tokenizer_len - 1 - k"
    assert np.array_equal(stage.decode_token_ids_to_actions(ids).numpy(), centres)
    ends = stage.decode_token_ids_to_actions(tokenize(np.array([-5.0, -1.0, 1.0, 5.0]))).numpy()
    assert np.array_equal(ends, centres[[0, 0, -1, -1]])
