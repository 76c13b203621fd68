#!/usr/bin/env python3
"""Generate tests/golden/token_metrics.npz: the four metrics the reference's native trainer commits after every micro-step
(prismatic/training/strategies/base_strategy.py:316-356) evaluated by the REFERENCE's own functions on seeded token ids.  CPU only;
run in the build container (the reference checkout does not exist on the GPU box).  The fixture is data (ids in, metric values
out); no reference source is copied.

Imported from the reference by path (skipping prismatic/__init__.py, as tools/make_golden.py does):
  prismatic/vla/constants.py, prismatic/training/train_utils.py (the two masks, compute_token_accuracy, compute_actions_l1_loss),
  prismatic/vla/action_tokenizer.py (ActionTokenizer.decode_token_ids_to_actions) - its logger import (and, where the installed
  transformers has no separate Qwen2 fast-tokenizer module, that import, used for one isinstance) is answered by a stub module,
  its base tokenizer by a stub object with vocab_size = 151643 (Qwen2.5's).

Cases: the whole [3, 95] batch and each sample alone.  Sample 2 holds 5 action tokens only: no next-actions row, so the
reference's next-actions accuracy (0 / 0) and L1 (l1_loss of empty tensors) are NaN there; every other value must be finite.

Usage: python tools/make_golden_token_metrics.py --ref <reference checkout> [--out tests/golden]
"""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch

TOKENIZER_LEN, N_BINS, L = 151643, 256, 95
BEGIN = TOKENIZER_LEN - (N_BINS + 1)


def import_reference(ref_root: str):
    sys.path.insert(0, ref_root)
    for name in ("prismatic", "prismatic.vla", "prismatic.training", "prismatic.overwatch"):
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(ref_root, *name.split("."))]
        sys.modules[name] = m
    ow = types.ModuleType("prismatic.overwatch.overwatch")
    ow.initialize_overwatch = lambda name: None               # (module-level logger of action_tokenizer.py; never called here)
    sys.modules["prismatic.overwatch.overwatch"] = ow
    fast = "transformers.models.qwen2.tokenization_qwen2_fast"
    try:
        importlib.import_module(fast)
    except ImportError:       # installed transformers without the separate fast-tokenizer module: action_tokenizer.py only isinstance()s it
        m = types.ModuleType(fast)
        m.Qwen2TokenizerFast = type("Qwen2TokenizerFast", (), {})
        sys.modules[fast] = m
    return {n.split(".")[-1]: importlib.import_module(n)
            for n in ("prismatic.vla.constants", "prismatic.training.train_utils", "prismatic.vla.action_tokenizer")}


def make_ids(seed: int = 20):
    """(pred_ids, gt_ids) int64 [3, 95] in the layout of batch['labels'][:, 1:]: IGNORE for the prompt, the prompt's last token (a
    valid non-action label), the action tokens, IGNORE padding behind a shorter prompt."""
    g = torch.Generator().manual_seed(seed)
    gt = torch.full((3, L), -100, dtype=torch.int64)
    n_act = [64, 64, 5]
    start = [30, 24, 40]                                      # ragged prompts: position of the prompt's last token
    for b in range(3):
        gt[b, start[b]] = int(torch.randint(0, BEGIN, (1,), generator=g))
        gt[b, start[b] + 1:start[b] + 1 + n_act[b]] = torch.randint(BEGIN + 1, TOKENIZER_LEN, (n_act[b],), generator=g)
    # the two extreme bins, on both sides of the current / next boundary
    gt[0, 31], gt[0, 32], gt[0, 40], gt[0, 41] = TOKENIZER_LEN - 1, BEGIN + 1, BEGIN + 2, TOKENIZER_LEN - 1
    gt[1, 25], gt[1, 60] = BEGIN + 1, TOKENIZER_LEN - 1
    pred = torch.randint(BEGIN + 1, TOKENIZER_LEN, (3, L), generator=g)          # (predictions exist at every position)
    hit = torch.rand(3, L, generator=g) < 0.45
    pred = torch.where(hit & (gt != -100), gt, pred)
    near = (torch.rand(3, L, generator=g) < 0.3) & ~hit & (gt > BEGIN)
    pred = torch.where(near, (gt + torch.randint(-3, 4, (3, L), generator=g)).clamp(BEGIN + 1, TOKENIZER_LEN - 1), pred)
    # predicted ids outside the action range: decodable through the clip only
    for (b, j), v in {(0, 33): 0, (0, 45): BEGIN, (0, 50): TOKENIZER_LEN, (0, 70): 151935,
                      (1, 26): 151935, (1, 27): 0, (1, 50): TOKENIZER_LEN, (1, 80): BEGIN,
                      (2, 41): 0, (2, 43): 151935, (0, 31): BEGIN + 1, (0, 32): TOKENIZER_LEN - 1, (1, 60): TOKENIZER_LEN - 1}.items():
        assert gt[b, j] > BEGIN
        pred[b, j] = v
    return pred, gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference checkout")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden"))
    args = ap.parse_args()
    R = import_reference(args.ref)
    C, TU, AT = R["constants"], R["train_utils"], R["action_tokenizer"]
    assert C.ACTION_TOKEN_BEGIN_IDX == BEGIN and C.ACTION_DIM == 7
    tok = AT.ActionTokenizer(types.SimpleNamespace(vocab_size=TOKENIZER_LEN), bins=N_BINS)
    assert tok.action_token_begin_idx == BEGIN
    pred, gt = make_ids()
    out = dict(pred_ids=pred.numpy(), gt_ids=gt.numpy(), tokenizer_len=np.int64(TOKENIZER_LEN), n_bins=np.int64(N_BINS),
               bin_centers=tok.bin_centers)
    names, values, counts = [], [], []
    for name, sl in (("all", slice(0, 3)), ("s0", slice(0, 1)), ("s1", slice(1, 2)), ("s2", slice(2, 3))):
        p, t = pred[sl], gt[sl]
        cur, nxt = TU.get_current_action_mask(t), TU.get_next_actions_mask(t)
        v = [float(TU.compute_token_accuracy(p, t, mask=cur)), float(TU.compute_actions_l1_loss(tok, p, t, mask=cur)),
             float(TU.compute_token_accuracy(p, t, mask=nxt)), float(TU.compute_actions_l1_loss(tok, p, t, mask=nxt))]
        names.append(name)
        values.append(v)
        counts.append([int(cur.sum()), int(nxt.sum())])
        print(name, counts[-1], v)
    values = np.asarray(values, dtype=np.float64)
    nan = np.isnan(values)
    assert nan.sum() == 2 and nan[3, 2] and nan[3, 3], "only sample 2's next-actions metrics may be NaN"
    assert np.isfinite(values[~nan]).all()
    assert counts[1] == [6, 58] and counts[2] == [6, 58] and counts[3] == [5, 0] and counts[0] == [17, 116]
    out.update(cases=np.asarray(names), metrics=values, mask_counts=np.asarray(counts, dtype=np.int64),
               current_mask=TU.get_current_action_mask(gt).numpy(), next_mask=TU.get_next_actions_mask(gt).numpy())
    path = os.path.join(args.out, "token_metrics.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
