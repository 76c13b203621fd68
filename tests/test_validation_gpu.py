"""GPU checks of the validation pass (--use_val_set, finetune.ValidationPass) on the plumbing-size configurations: training is
untouched by it, its numbers are the checkpointed model's, the pipelined adapter step survives it, frames are never augmented,
the time limit and the shape contract hold, and two ranks validate on their own."""
import glob
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


def _cfg(backbone):
    from vla_adapter_amd import engine as E
    mcfg = E.NAMED_CONFIGS[backbone]()
    mcfg.n_img = 2 if backbone == "tiny_fused" else 1
    mcfg.pro = True
    return mcfg


def _batches(backbone, n, seed0, B=4):
    from vla_adapter_amd import synthetic as S
    return [S.make_batch(_cfg(backbone), B, DEV, seed=seed0 + i, P=32 if backbone == "tiny" else 24, ragged=True) for i in range(n)]


def _L(*lists):
    return max(b["input_ids"].shape[1] for bs in lists for b in bs)


MODES = {"adapter": ["--use_fz", "True"], "lora": ["--use_lora", "True", "--lora_rank", "8", "--lora_dropout", "0.1"], "full": []}


def _args(backbone, mode, graph, tmp, L, extra=(), B=4, max_steps=4, save_freq=1000):
    return (["--tiny", "true", "--backbone", backbone, "--num_images_in_input", "2" if backbone == "tiny_fused" else "1", "--batch_size", str(B),
             "--max_steps", str(max_steps), "--learning_rate", "1e-3", "--wandb_log_freq", "1", "--save_freq", str(save_freq), "--phase", "Training",
             "--use_proprio", "True", "--use_graph", graph, "--max_seq_len", str(L), "--run_root_dir", str(tmp), "--run_id_override", "r"]
            + MODES[mode] + list(extra))


def _ckpt(d):
    """Every tensor of a checkpoint directory, keyed by file and name."""
    from safetensors.torch import load_file
    out = {}
    for f in sorted(glob.glob(os.path.join(d, "**", "*"), recursive=True)):
        if f.endswith(".pt"):
            out.update({(os.path.relpath(f, d), k): v for k, v in torch.load(f, weights_only=True).items()})
        elif f.endswith(".safetensors"):
            out.update({(os.path.relpath(f, d), k): v for k, v in load_file(f).items()})
    assert out
    return out


def _recompute(backbone, mode, d, step, val, L, rank=0, seed=0, phase_training=True):
    """Load the checkpoint of `step` into a fresh engine / trainer and recompute every validation batch eagerly (forward + the
    L1 loss, no dropout, the reproduced validation noise) in the sweep's order; the reference's mean over batches."""
    from vla_adapter_amd import checkpoints as CK, engine as E, finetune as F, ops, synthetic as S
    from safetensors.torch import load_file
    mcfg = _cfg(backbone)
    W = S.make_weights(mcfg, DEV, seed=seed)
    W["head"], W["proprio"], W["action_queries"] = CK.load_run_dir(d, step, with_action_queries=True)
    eng = E.VLAEngine(mcfg, W, DEV)
    model = eng
    if mode == "lora":
        from vla_adapter_amd.trainers import LoRAFinetune
        model = LoRAFinetune(eng, rank=8, seed=seed, dropout=0.0)
        model.load_lora_state_dict(load_file(os.path.join(d, "lora_adapter", "adapter_model.safetensors")))
    pad = min(S.PAD_ID, mcfg.llm.vocab - 1)
    n = len(val)
    vals = []
    for j, i in enumerate(list(range(rank % n, n)) + list(range(rank % n))):
        b = F.pad_to(val[i], L, pad)
        noise = F.validation_noise(F.FinetuneConfig(seed=seed), mcfg, rank, step, j).to(DEV) if phase_training else None
        pred = model.forward(b, noise)
        vals.append(ops.l1_loss(pred, eng._to_bf16(b["actions"]), want_grad=False)[0].tolist())
    mean = [sum(v[k] for v in vals) / len(vals) for k in range(3)]
    return dict(step=step, loss_value=mean[0], loss=mean[0], curr_action_l1_loss=mean[1], next_actions_l1_loss=mean[2], val_batches_count=len(vals))


def _close(got, want, rel):
    assert got["step"] == want["step"] and got["val_batches_count"] == want["val_batches_count"], (got, want)
    for k in ("loss_value", "loss", "curr_action_l1_loss", "next_actions_l1_loss"):
        if rel == 0:
            assert got[k] == want[k], (k, got, want)
        else:
            assert abs(got[k] - want[k]) <= rel * abs(want[k]), (k, got, want)


# 1 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backbone,mode,graph", [("tiny", "adapter", "true"), ("tiny", "adapter", "false"), ("tiny_fused", "adapter", "true"),
                                                 ("tiny", "lora", "true"), ("tiny_fused", "lora", "true"), ("tiny", "lora", "false"),
                                                 ("tiny", "full", "true")])
def test_training_is_bit_identical_with_and_without_validation(tmp_path, backbone, mode, graph):
    from vla_adapter_amd import finetune as F
    train, val = _batches(backbone, 3, 400), _batches(backbone, 2, 420)
    L = _L(train, val)
    a = F.finetune(F.parse_args(_args(backbone, mode, graph, tmp_path / "a", L, ["--use_val_set", "True", "--val_freq", "2"])), batches=train,
                   val_batches=val)
    b = F.finetune(F.parse_args(_args(backbone, mode, graph, tmp_path / "b", L)), batches=train)
    assert [v["step"] for v in a["val_log"]] == [2, 4] and all(v["val_batches_count"] == 2 for v in a["val_log"])
    assert all(v[k] == v[k] and v[k] > 0 for v in a["val_log"] for k in ("loss_value", "curr_action_l1_loss", "next_actions_l1_loss"))
    assert a["log"] == b["log"] and "val_log" in b and b["val_log"] == []
    ca, cb = _ckpt(str(tmp_path / "a" / "r--4_chkpt")), _ckpt(str(tmp_path / "b" / "r--4_chkpt"))
    assert set(ca) == set(cb) and all(torch.equal(ca[k], cb[k]) for k in ca), [k for k in ca if not torch.equal(ca[k], cb[k])][:5]


# 2 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backbone,mode,graph", [("tiny", "adapter", "false"), ("tiny", "adapter", "true"), ("tiny_fused", "adapter", "true"),
                                                 ("tiny", "lora", "false"), ("tiny", "lora", "true")])
def test_val_log_is_the_checkpointed_models_mean(tmp_path, backbone, mode, graph):
    from vla_adapter_amd import finetune as F
    train, val = _batches(backbone, 2, 440), _batches(backbone, 3, 460)
    L = _L(train, val)
    out = F.finetune(F.parse_args(_args(backbone, mode, graph, tmp_path, L, ["--use_val_set", "True", "--val_freq", "2"], save_freq=2)),
                     batches=train, val_batches=val)
    assert [v["step"] for v in out["val_log"]] == [2, 4]
    for v in out["val_log"]:
        want = _recompute(backbone, mode, str(tmp_path / f"r--{v['step']}_chkpt"), v["step"], val, L)
        _close(v, want, 0 if graph == "false" else 1e-6)
    assert out["val_log"][0]["loss_value"] != out["val_log"][1]["loss_value"]


# 3 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phase", ["Training", "Inference"])
def test_pipelined_adapter_step_survives_a_sweep_every_step(tmp_path, phase):
    """The captured adapter step keeps the next batch's vision stage and its update in flight between calls: a sweep after
    every step must leave the training losses exactly as they are without one (three distinct training batches)."""
    from vla_adapter_amd import finetune as F
    train, val = _batches("tiny", 3, 480), _batches("tiny", 2, 490)
    L = _L(train, val)
    extra = ["--phase", phase, "--max_steps", "5"]
    a = F.finetune(F.parse_args(_args("tiny", "adapter", "true", tmp_path / "a", L, extra + ["--use_val_set", "True", "--val_freq", "1"])),
                   batches=train, val_batches=val)
    b = F.finetune(F.parse_args(_args("tiny", "adapter", "true", tmp_path / "b", L, extra)), batches=train)
    assert [v["step"] for v in a["val_log"]] == [1, 2, 3, 4, 5]
    la = [(l["loss_value"], l["curr_action_l1_loss"], l["next_actions_l1_loss"]) for l in a["log"]]
    assert la == [(l["loss_value"], l["curr_action_l1_loss"], l["next_actions_l1_loss"]) for l in b["log"]]
    assert len({x[0] for x in la[:3]}) == 3, "the three training batches must differ for the check to mean anything"


# 4 ----------------------------------------------------------------------------------------------------------------------
def _frames(backbone, batches, seed0):
    mcfg = _cfg(backbone)
    out = []
    for i, b in enumerate(batches):
        b = {k: v for k, v in b.items() if k != "pixel_values"}
        g = torch.Generator().manual_seed(seed0 + i)
        B = b["input_ids"].shape[0]
        b["frames_u8"] = torch.randint(0, 256, (B, mcfg.n_img, mcfg.vit[0].img, mcfg.vit[0].img, 3), generator=g, dtype=torch.uint8)
        out.append(b)
    return out


@pytest.mark.parametrize("backbone,mode,graph", [("tiny", "adapter", "true"), ("tiny_fused", "adapter", "false"), ("tiny", "lora", "true")])
def test_frame_validation_batches_are_never_augmented(tmp_path, backbone, mode, graph):
    from vla_adapter_amd import finetune as F
    from vla_adapter_amd.input_stage import GPUInputStage, backbone_norms
    mcfg = _cfg(backbone)
    train = _frames(backbone, _batches(backbone, 2, 500), 500)          # augmented training frames: --image_aug is in force
    vf = _frames(backbone, _batches(backbone, 2, 510), 510)
    st = GPUInputStage(DEV, backbones=backbone_norms(mcfg), image_size=mcfg.vit[0].img)
    vp = [dict({k: v for k, v in b.items() if k != "frames_u8"}, pixel_values=st.pixels(b["frames_u8"].to(DEV))) for b in vf]
    L = _L(train, vf)
    extra = ["--image_aug", "True", "--use_val_set", "True", "--val_freq", "2"]
    a = F.finetune(F.parse_args(_args(backbone, mode, graph, tmp_path / "a", L, extra)), batches=train, val_batches=vf)
    b = F.finetune(F.parse_args(_args(backbone, mode, graph, tmp_path / "b", L, extra)), batches=train, val_batches=vp)
    assert len(a["val_log"]) == 2 and a["val_log"] == b["val_log"] and a["log"] == b["log"]


# 5 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["true", "false"])
def test_time_limit_batch_count_and_shape_contract(tmp_path, graph):
    from vla_adapter_amd import finetune as F
    train, val = _batches("tiny", 2, 530), _batches("tiny", 3, 540)
    L = _L(train, val)
    common = ["--use_val_set", "True", "--val_freq", "2", "--max_steps", "2"]
    out = F.finetune(F.parse_args(_args("tiny", "adapter", graph, tmp_path / "a", L, common + ["--val_time_limit", "0"])), batches=train, val_batches=val)
    assert [v["val_batches_count"] for v in out["val_log"]] == [1]
    out = F.finetune(F.parse_args(_args("tiny", "adapter", graph, tmp_path / "b", L, common)), batches=train, val_batches=val)
    assert [v["val_batches_count"] for v in out["val_log"]] == [3]                     # one pass: the finite source is not cycled
    with pytest.raises(ValueError, match="batch size"):
        F.finetune(F.parse_args(_args("tiny", "adapter", graph, tmp_path / "c", L, common)), batches=train, val_batches=_batches("tiny", 1, 550, B=3))


def test_val_batch_file_directory_and_the_command_line(tmp_path):
    """--val_batch_file as a directory of .pt dicts through the script entry point: JSON validation lines at steps 5 and 10."""
    from vla_adapter_amd import finetune as F
    train, val = _batches("tiny", 2, 560), _batches("tiny", 2, 570)
    L = _L(train, val)
    for name, bs in (("train", train), ("val", val)):
        os.makedirs(tmp_path / name)
        for i, b in enumerate(bs):
            torch.save({k: v.cpu() for k, v in F.pad_to(b, L, 0).items()}, tmp_path / name / f"{i:03d}.pt")
    r = subprocess.run([sys.executable, os.path.join("vla-scripts", "finetune.py"), "--tiny", "true", "--use_fz", "True", "--use_proprio", "True",
                        "--batch_size", "4", "--batch_file", str(tmp_path / "train"), "--use_val_set", "True", "--val_batch_file", str(tmp_path / "val"),
                        "--val_freq", "5", "--max_steps", "10", "--save_freq", "1000", "--run_root_dir", str(tmp_path / "runs")],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    vl = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{") and "val_batches_count" in l]
    assert [v["step"] for v in vl] == [5, 10] and all(v["val_batches_count"] == 2 for v in vl), r.stdout[-3000:]


# 6 ----------------------------------------------------------------------------------------------------------------------
def test_two_ranks_validate_on_their_own(tmp_path):
    """Two gloo ranks on one GPU (tools/validation_two_ranks.py): each rank's val_log is its own single-process recomputation
    (its own offset into the held-out batches, its own noise), and training is what it is without validation."""
    from vla_adapter_amd import engine as E, synthetic as S
    cfg = E.tiny_config()
    mk = lambda n, s0: [S.make_batch(cfg, 4, DEV, seed=s0 + i, P=32, ragged=True) for i in range(n)]
    val = mk(3, 720)
    L = _L(mk(3, 700), val)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, VLA_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join("tools", "validation_two_ranks.py"), str(tmp_path), str(L)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("validation-two-ranks-ok") == 2, r.stdout[-3000:]
    logs = [json.load(open(tmp_path / f"rank{k}.json")) for k in range(2)]
    for rank, lg in enumerate(logs):
        assert lg["world"] == 2 and lg["log"] == lg["plain_log"]
        assert [v["step"] for v in lg["val_log"]] == [2, 4]
        for v in lg["val_log"]:
            want = _recompute("tiny", "adapter", str(tmp_path / "val" / f"r--{v['step']}_chkpt"), v["step"], val, L, rank=rank)
            _close(v, want, 1e-6)
    assert logs[0]["val_log"] != logs[1]["val_log"]
