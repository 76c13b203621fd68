#!/usr/bin/env python3
"""Times the two passes of the fused image augmentation (vla_augment_stats, vla_augment_apply with every op on and in-kernel
draws) with device events after warm-up, at the shipped recipe's shape (B = 8) and the headline shape (B = 32): two images per
sample, DINOv2 + SigLIP normalisation (6 output channels per image), 224 x 224, bf16 output.  Bytes are computed from the shapes:
the statistics pass reads the uint8 frames once, the apply pass reads them again and writes the bf16 pixel tensor.  Prints one
JSON line per shape with microseconds per call and achieved GB/s against the HBM roof (6.3 TB/s achievable, 8.0 TB/s spec)."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from vla_adapter_amd import ops  # noqa: E402
from vla_adapter_amd.input_stage import IMAGENET_MEAN, IMAGENET_STD, SIGLIP_MEAN, SIGLIP_STD, ImageAugment  # noqa: E402

HBM_ACHIEVABLE = 6.3e12


def run(B: int, n_img: int, size: int, iters: int, warmup: int) -> dict:
    dev = "cuda"
    N, H, W, nb = B * n_img, size, size, 2
    lib = ops._lib()
    fr = torch.randint(0, 256, (B, n_img, H, W, 3), device=dev, dtype=torch.uint8)
    out = torch.empty(B, 3 * nb * n_img, H, W, device=dev, dtype=torch.bfloat16)
    params = torch.empty(N, ops.AUG_NPARAM, device=dev, dtype=torch.float32)
    slab = torch.empty(lib.vla_augment_slab_floats(N, H, W), device=dev, dtype=torch.float32)
    aug = ImageAugment()
    mask, cfg = aug.mask(), (C.c_float * 7)(*aug.cfg7())
    mean = (C.c_float * 6)(*IMAGENET_MEAN, *SIGLIP_MEAN)
    std = (C.c_float * 6)(*IMAGENET_STD, *SIGLIP_STD)

    def stats(step):
        ops.N.check(lib.vla_augment_stats(ops._st(), ops._p(fr), ops._p(params), ops._p(slab), N, H, W, n_img, mask, cfg, 0, 0, step), "stats")

    def apply(step):
        ops.N.check(lib.vla_augment_apply(ops._st(), ops._p(fr), ops._p(params), ops._p(slab), ops._p(out), None, N, H, W, n_img, nb, mean, std,
                                          0, mask, cfg, 0, 0, step), "apply")

    def timed(fn):
        for i in range(warmup):
            fn(i)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters          # us per call

    def both(i):
        stats(i)
        apply(i)
    t_stats, t_apply, t_both = timed(stats), timed(apply), timed(both)
    u8 = N * H * W * 3
    bytes_stats, bytes_apply = u8, u8 + out.numel() * 2
    gbs = lambda b, t: b / (t * 1e-6) / 1e9
    return dict(B=B, n_img=n_img, size=size, backbones=nb, us_stats=round(t_stats, 2), us_apply=round(t_apply, 2), us_both=round(t_both, 2),
                gbps_stats=round(gbs(bytes_stats, t_stats), 1), gbps_apply=round(gbs(bytes_apply, t_apply), 1),
                gbps_both=round(gbs(bytes_stats + bytes_apply, t_both), 1),
                share_of_hbm_roof_both=round((bytes_stats + bytes_apply) / HBM_ACHIEVABLE / (t_both * 1e-6), 3),
                mbytes_stats=round(bytes_stats / 1e6, 2), mbytes_apply=round(bytes_apply / 1e6, 2))


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_augment needs a GPU"
    for B in (8, 32):
        print(json.dumps(run(B, 2, 224, args.iters, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
