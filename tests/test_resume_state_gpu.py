"""--save_train_state / --resume_train_state / --log_state_digest on the device (vla_adapter_amd/train_state.py).

Per case one straight run - ``--save_freq 3 --max_steps 6 --save_train_state True --log_state_digest True --wandb_log_freq 1`` - and a
second finetune() call, with a fresh engine, that resumes from the step-3 checkpoint and runs to 6.  Every comparison is an equality:
the log lines behind step 3 (losses, learning rate, gradient norm, token metrics and the state_digest strings), the validation entries
behind step 3, every flat data / m / v buffer at the end (torch.equal), and the state file both runs write at step 6.  One further
case resumes the same checkpoint the reference's way (plain --resume) and must NOT reproduce the digests: the suite discriminates."""
import json

import pytest
import torch

from tests.test_heldout_gpu import FRACTION, L, _tables_a, _tables_b
from vla_adapter_amd import train_state as TS

pytestmark = pytest.mark.gpu

ADAPTER = ["--use_fz", "True"]
LORA = ["--use_lora", "True", "--lora_rank", "8"]
CASES = {
    "adapter-captured": ADAPTER + ["--use_graph", "true"],
    "adapter-eager": ADAPTER + ["--use_graph", "false"],
    "adapter-ga2-clip": ADAPTER + ["--use_graph", "true", "--grad_accumulation_steps", "2", "--max_grad_norm", "1.0"],
    "lora-dropout": LORA + ["--use_graph", "true", "--lora_dropout", "0.1"],
    "full": ["--use_graph", "true"],
    "lora-token-ce": LORA + ["--use_graph", "true", "--objective", "token_ce"],
    "episodes-aug-heldout": ADAPTER + ["--use_graph", "true", "--conservative_rows", "true", "--max_seq_len", str(L), "--image_aug", "True",
                                       "--use_val_set", "True", "--val_episode_fraction", str(FRACTION), "--val_freq", "3"],
    "episode-mix": ADAPTER + ["--use_graph", "true", "--conservative_rows", "true", "--max_seq_len", str(L), "--image_aug", "True"],
}


def _args(tmp, case, extra=()):
    src = []
    if case == "episodes-aug-heldout":
        src = ["--episode_file", str(tmp / "suite_a.pt")]
    elif case == "episode-mix":
        src = ["--episode_mix", f"{tmp / 'suite_a.pt'}=1.0,{tmp / 'suite_b.pt'}=0.5"]
    return (["--tiny", "true", "--backbone", "tiny", "--batch_size", "4", "--max_steps", "6", "--save_freq", "3", "--learning_rate", "1e-3", "--lr_warmup_steps", "8",
             "--wandb_log_freq", "1", "--phase", "Training", "--use_proprio", "True", "--seed", "5", "--run_id_override", "r",
             "--save_train_state", "True", "--log_state_digest", "True"] + CASES[case] + src + list(extra))


def _flat(store):
    def grab(eng, trainer):
        for name, P in (trainer or eng)._state_buffers():
            for part in TS.PARTS:
                store[f"{name}.{part}"] = getattr(P, part).detach().clone()
    return grab


_STRAIGHT = {}


def straight(case, tmp_path_factory):
    """The straight run of a case, made once (the plain-resume case shares adapter-captured's)."""
    if case not in _STRAIGHT:
        from vla_adapter_amd import finetune as F
        tmp = tmp_path_factory.mktemp(case.replace("-", "_"))
        if case.startswith("episode"):
            torch.save(_tables_a(), tmp / "suite_a.pt")
            torch.save(_tables_b(), tmp / "suite_b.pt")
        flat = {}
        out = F.finetune(F.parse_args(_args(tmp, case, ["--run_root_dir", str(tmp / "a")])), on_finish=_flat(flat))
        _STRAIGHT[case] = (tmp, out, flat)
    return _STRAIGHT[case]


def _resume_args(tmp, case, extra=()):
    return _args(tmp, case, ["--run_root_dir", str(tmp / "b"), "--resume", "True", "--resume_step", "3", "--resum_vla_path", str(tmp / "a" / "r--3_chkpt"),
                             *extra])


def _same(x, y):
    if isinstance(x, torch.Tensor):
        return isinstance(y, torch.Tensor) and x.dtype == y.dtype and torch.equal(x, y)
    if isinstance(x, dict):
        return isinstance(y, dict) and x.keys() == y.keys() and all(_same(x[k], y[k]) for k in x)
    return x == y


@pytest.mark.parametrize("case", list(CASES))
def test_a_resumed_run_goes_on_bit_for_bit(case, tmp_path_factory):
    """The state equalities come first, the float equality of the log lines last (lora-token-ce: the loss sum is taken in a fixed
    order, vla_token_ce_metrics_ordered - with the atomic sum the state was equal and the reported loss differed in its last bit)."""
    from vla_adapter_amd import finetune as F
    tmp, a, flat_a = straight(case, tmp_path_factory)
    ga2 = case == "adapter-ga2-clip"
    assert [l["step"] for l in a["log"]] == list(range(6 if ga2 else 7)), "one line per gradient step"
    # the state file of step 3: loadable without pickle, nothing in it but tensors, ints, strings and containers of them
    st = torch.load(tmp / "a" / "r--3_chkpt" / "train_state--3_checkpoint.pt", weights_only=True)
    assert st["version"] == TS.FORMAT_VERSION and st["log_step"] == 3 and st["next_grad_step"] == 4 and st["next_micro_step"] == (8 if ga2 else 4)
    assert st["mode"] == a["mode"] and set(st["buffers"]) == ({"head"} if a["mode"] == "adapter" else {"head", "backbone"})
    assert list(st["step_counts"].values()) == [4] and json.loads(st["fingerprint"])["seed"] == 5
    assert st["buffers"]["head"]["digest"] == a["log"][3]["state_digest"]["head"], "the state holds the digests the log line of step 3 reported"
    assert ("drop_step" in st["counters"]) == (a["mode"] == "lora")
    if case == "lora-dropout":
        assert st["counters"]["drop_step"] == 2 + 4, "two warm-up passes of capture() and four steps"
    assert not any(k.startswith("model") or "weight" in k for k in st), "the weights are not stored twice"

    flat_b = {}
    b = F.finetune(F.parse_args(_resume_args(tmp, case, ["--resume_train_state", "True"])), on_finish=_flat(flat_b))
    tail = [l for l in a["log"] if l["step"] > 3]
    assert len(tail) == (2 if ga2 else 3) and [l["step"] for l in b["log"]] == [l["step"] for l in tail]
    for la, lb in zip(tail, b["log"]):
        assert la["state_digest"] == lb["state_digest"], f"step {la['step']}: {la['state_digest']} != {lb['state_digest']}"
        assert la["lr"] == lb["lr"] == F.lr_at(la["step"], F.parse_args(_args(tmp, case))), "the warm-up ramp goes on, it does not start again"
    assert len({json.dumps(l["state_digest"], sort_keys=True) for l in a["log"]}) == len(a["log"]), "every step moved the state"
    assert all(l["loss_value"] == l["loss_value"] for l in a["log"])
    if ga2:
        assert all("grad_norm" in l for l in b["log"])
    if case == "lora-token-ce":
        from vla_adapter_amd.ops import TOKEN_METRIC_NAMES
        assert all(set(TOKEN_METRIC_NAMES) <= set(l) for l in b["log"])
    assert flat_a.keys() == flat_b.keys() and len(flat_a) == 3 * len(st["buffers"])
    for k in flat_a:
        assert torch.equal(flat_a[k], flat_b[k]), f"{k} differs after the resumed run"
    assert [v for v in a["val_log"] if v["step"] > 3] == b["val_log"]
    if case == "episodes-aug-heldout":
        assert [v["step"] for v in a["val_log"]] == [3, 6] and [v["step"] for v in b["val_log"]] == [6]
    assert b["final_step"] == a["final_step"] == 6
    if not ga2:                # both runs saved at step 6, state included: equal in every entry (moments, generator, counters, digests, fingerprint)
        sa = torch.load(tmp / "a" / "r--6_chkpt" / "train_state--6_checkpoint.pt", weights_only=True)
        sb = torch.load(tmp / "b" / "r--6_chkpt" / "train_state--6_checkpoint.pt", weights_only=True)
        assert sa["next_micro_step"] == 7 and _same(sa, sb), [k for k in sa if not _same(sa[k], sb.get(k))]
        assert sa["buffers"]["head"]["digest"] == a["log"][-1]["state_digest"]["head"]
    else:                      # the run ended inside gradient step 6: the weights are saved, a state is not
        assert not list((tmp / "a").rglob("train_state--6_checkpoint.pt")) and not list((tmp / "b").rglob("train_state--6_checkpoint.pt"))
        assert (tmp / "a" / "r--6_chkpt" / "action_head--6_checkpoint.pt").exists()
    # last, what the state equalities above do not already imply: every logged number as a float (losses, metrics, gradient norm)
    for la, lb in zip(tail, b["log"]):
        assert la == lb, f"step {la['step']}: {la} != {lb}"


def test_plain_resume_does_not_reproduce_the_digests(tmp_path_factory):
    """The reference's --resume from the same checkpoint: the weights come back, the moments, the warm-up position, the stream and
    the generators start over - the digests behind step 3 differ from the straight run's, at every step and in every buffer part."""
    from vla_adapter_amd import finetune as F
    tmp, a, _ = straight("adapter-captured", tmp_path_factory)
    c = F.finetune(F.parse_args(_resume_args(tmp, "adapter-captured", ["--run_root_dir", str(tmp / "c")])))
    assert [l["step"] for l in c["log"]] == [3, 4, 5, 6], "log_step = resume_step + gradient step, from 0"
    by_step = {l["step"]: l for l in a["log"]}
    for l in c["log"]:
        if l["step"] > 3:
            for part in TS.PARTS:
                assert l["state_digest"]["head"][part] != by_step[l["step"]]["state_digest"]["head"][part], (l["step"], part)
    assert [l["lr"] for l in c["log"]] == [by_step[g]["lr"] for g in range(4)] and c["log"][1]["lr"] != by_step[4]["lr"], "the warm-up ramp runs again"


def test_a_resume_refuses_other_weights_and_other_flags(tmp_path_factory):
    """The refusals that need the device: weights that are not the recorded ones (the step-6 files under the step-3 state), and - before
    any weight is loaded - flags that differ, a step that differs, a directory without a state file."""
    import shutil
    from vla_adapter_amd import finetune as F
    tmp, a, _ = straight("adapter-captured", tmp_path_factory)
    with pytest.raises(ValueError, match=r"trajectory differ.*seed: recorded 5, now 6"):
        F.finetune(F.parse_args([x if x != "5" else "6" for x in _resume_args(tmp, "adapter-captured", ["--resume_train_state", "True"])]))
    mixed = tmp / "mixed"
    shutil.copytree(tmp / "a" / "r--6_chkpt", mixed)
    for f in mixed.glob("*--6_checkpoint.pt"):
        f.rename(mixed / f.name.replace("--6_checkpoint", "--3_checkpoint"))
    shutil.copy(tmp / "a" / "r--3_chkpt" / "train_state--3_checkpoint.pt", mixed / "train_state--3_checkpoint.pt")
    args = _resume_args(tmp, "adapter-captured", ["--resume_train_state", "True", "--run_root_dir", str(tmp / "d")])
    args[args.index("--resum_vla_path") + 1] = str(mixed)
    with pytest.raises(ValueError, match="loaded weights are not the ones the state was written beside.*head.data"):
        F.finetune(F.parse_args(args))
    bare = tmp / "bare"
    shutil.copytree(tmp / "a" / "r--3_chkpt", bare)
    (bare / "train_state--3_checkpoint.pt").unlink()
    args[args.index("--resum_vla_path") + 1] = str(bare)
    with pytest.raises(ValueError, match="no state file"):
        F.finetune(F.parse_args(args))


def _two_ranks(out_dir, args):
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, VLA_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out_dir.mkdir()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join("tools", "resume_two_ranks.py"), str(out_dir)] + list(args),
                       cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("resume-two-ranks-ok") == 2, r.stdout[-3000:]
    return [json.load(open(out_dir / f"rank{k}.json")) for k in range(2)], [torch.load(out_dir / f"rank{k}_flat.pt", weights_only=True) for k in range(2)]


def test_two_ranks_resume_from_the_file_rank_0_wrote(tmp_path):
    """Two gloo ranks on one GPU (tools/resume_two_ranks.py), adapter-only, captured: rank 0 writes the state, both ranks read it; each
    keeps its own generator seed and takes the recorded offset.  Per rank the log lines behind step 3 and the final buffers equal the
    straight two-rank run's, and the ranks' parameters and moments equal each other."""
    args = _args(tmp_path, "adapter-captured")
    logs_a, flat_a = _two_ranks(tmp_path / "a", args)
    logs_b, flat_b = _two_ranks(tmp_path / "b", args + ["--resume", "True", "--resume_step", "3", "--resum_vla_path", str(tmp_path / "a" / "run0" / "r--3_chkpt"),
                                                        "--resume_train_state", "True"])
    st = torch.load(tmp_path / "a" / "run0" / "r--3_chkpt" / "train_state--3_checkpoint.pt", weights_only=True)
    assert json.loads(st["fingerprint"])["world_size"] == 2 and not list((tmp_path / "a" / "run1").rglob("train_state--*")), "rank 0 writes"
    for k in range(2):
        tail = [l for l in logs_a[k]["log"] if l["step"] > 3]
        assert logs_a[k]["world"] == 2 and len(tail) == 3 and tail == logs_b[k]["log"], f"rank {k}"
        assert flat_a[k].keys() == flat_b[k].keys() and all(torch.equal(flat_a[k][n], flat_b[k][n]) for n in flat_a[k]), f"rank {k}"
    assert all(torch.equal(flat_b[0][n], flat_b[1][n]) for n in flat_b[0]), "the ranks stay in sync"
    assert logs_a[0]["log"][4]["loss_value"] != logs_a[1]["log"][4]["loss_value"], "every rank trains on its own batches and noise"
    assert logs_a[0]["log"][4]["state_digest"] == logs_a[1]["log"][4]["state_digest"]
