#!/usr/bin/env python3
"""Records what the serving calls compute on fixed inputs, so that two versions of the engine can be compared bit for bit: the sibling
of tools/finetune_trajectory.py for predict_action / predict_actions / generate_actions, which no fine-tune run reaches.

At ``--tiny`` (the only size), from fixed seeds, on ONE model: predict_action at B = 1, predict_actions at two (B, L), generate_actions at
T = 8 - then all three again in reverse order, so that every call replays its graphs behind a call of another shape.  Per call the
record holds the sha256 of the actions, of the action hidden states and of the tokens.  ``max_memory_allocated`` is recorded and not
compared.

  python tools/serve_trajectory.py --tiny --out new.json [--label <commit>]    # on a GPU; vla_adapter_amd is taken from beside tools/
  python tools/serve_trajectory.py --compare parent.json new.json                # one JSON line: identical, and what differs
"""
import argparse
import hashlib
import json

import _episode_bench as EB          # (puts the tree beside tools/ on sys.path)
import numpy as np
import torch

STATS = {"libero": {"action": {"q01": np.linspace(-0.9, -0.3, 7).tolist(), "q99": np.linspace(0.4, 1.3, 7).tolist(), "min": [-1.0] * 7,
                               "max": [1.5] * 7, "mask": [True] * 6 + [False]}}}
SERVE = {"b2_l96": [20, 27], "b3_l128": [40, 33, 25]}        # prompt lengths; + 65 ids rounded up to 32: L = 96 and 128


def sha(x) -> str:
    a = x.detach().cpu().contiguous().view(torch.uint8).numpy() if isinstance(x, torch.Tensor) else np.ascontiguousarray(x)
    return hashlib.sha256(f"{a.dtype}{a.shape}".encode() + a.tobytes()).hexdigest()


def record() -> dict:
    from vla_adapter_amd import engine as E, synthetic as S
    from vla_adapter_amd.modeling_prismatic import OpenVLAForActionPrediction
    cfg, dev = E.tiny_config(), "cuda"
    vla = OpenVLAForActionPrediction(cfg, S.make_weights(cfg, dev, seed=7, std=0.05), dev, norm_stats=STATS)
    g = torch.Generator().manual_seed(8)
    ids = lambda lens: [torch.randint(0, cfg.llm.vocab - 300, (n,), generator=g).tolist() for n in lens]
    px = lambda B: torch.randn(B, 3, cfg.vit[0].img, cfg.vit[0].img, generator=g).clamp_(-3, 3).to(torch.bfloat16).to(dev)
    pr = lambda B: (torch.rand(B, 8, generator=g) * 2 - 1).numpy()
    one = dict(ids=torch.tensor(ids([24])), px=px(1), pr=pr(1)[0])
    serve = {k: dict(ids=ids(lens), px=px(len(lens)), pr=pr(len(lens))) for k, lens in SERVE.items()}
    gen = dict(ids=ids([20, 17, 25]), px=px(3))

    def predict_action():
        a, hid = vla.predict_action(input_ids=one["ids"], proprio=one["pr"], proprio_projector=True, action_head=True, pixel_values=one["px"],
                                    attention_mask=torch.ones_like(one["ids"], dtype=torch.bool))
        return dict(actions=sha(a), hidden=sha(hid))

    def predict_actions(k):
        a, hid = vla.predict_actions(serve[k]["ids"], pixel_values=serve[k]["px"], proprio=serve[k]["pr"], proprio_normalized=True)
        return dict(actions=sha(a), hidden=sha(hid))

    def generate_actions():
        _, tok = vla.generate_actions(gen["ids"], pixel_values=gen["px"], max_new_tokens=8, return_tokens=True)
        return dict(tokens=sha(tok))
    calls = [("predict_action", predict_action)] + [(k, lambda k=k: predict_actions(k)) for k in SERVE] + [("generate_actions", generate_actions)]
    out = {f"{name}.{rnd}": fn() for rnd, order in enumerate((calls, calls[::-1])) for name, fn in order}
    torch.cuda.synchronize()
    return dict(calls=out, graphs=len(vla.engine._predict_graphs), max_memory_allocated=torch.cuda.max_memory_allocated())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tiny", action="store_true", help="the plumbing-size configuration (the only one: accepted for symmetry)")
    ap.add_argument("--out", help="where the record is written")
    ap.add_argument("--label", default=None, help="recorded as it is: the commit the engine is of")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        a, b = (json.load(open(p)) for p in args.compare)
        differing = sorted(k for k in set(a["calls"]) | set(b["calls"]) if a["calls"].get(k) != b["calls"].get(k))
        differing += ["graphs"] if a["graphs"] != b["graphs"] else []
        print(json.dumps(dict(identical=not differing, calls=len(a["calls"]), labels=[a.get("label"), b.get("label")], differing=differing,
                              max_memory_allocated=[a["max_memory_allocated"], b["max_memory_allocated"]])), flush=True)
        return
    assert args.out, "--out or --compare"
    assert torch.cuda.is_available(), "serve_trajectory needs a GPU"
    json.dump(dict(label=args.label, device=torch.cuda.get_device_name(0), **record()), open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
