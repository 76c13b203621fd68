#!/usr/bin/env python3
"""Converts a raw episode file (``frames_u8``) into the JPEG form (``frames_jpeg``, ``frame_off``, ``frame_shape``:
vla_adapter_amd/jpeg_store.py) with Pillow, and prints the byte ratio as one JSON line.

This is LOSSY: every frame is encoded anew at ``--quality``.  It is meant for users who hold arrays; users who hold the encoded
files of their dataset (baseline JPEG, 4:2:0 or 4:4:4, sides that are multiples of 16) write the three keys directly and lose nothing.

``--restart_rows r`` (default 1) puts a restart marker behind every r rows of MCUs: the decode then has one independent segment per
interval instead of one per image, which is what makes it fast on the device; 0 writes none.  The markers cost
a few bytes per interval.

  python tools/pack_episodes_jpeg.py episodes.pt episodes_jpeg.pt --quality 95 --subsampling 4:2:0 --restart_rows 1

``--device cuda`` codes the frames on the device instead (vla_adapter_amd/jpeg_store.py: encode_tables) and writes
the same file, byte for byte; it takes 4:2:0 and --restart_rows >= 1 only.  The default, ``--device cpu``, is the Pillow path above.
"""
import argparse
import io
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

SUBSAMPLING = {"4:2:0": 2, "4:4:4": 0}


def pack(d: dict, quality: int = 95, subsampling: str = "4:2:0", restart_rows: int = 1) -> dict:
    """The episode dict ``d`` with its frames_u8 [T, n_img, H, W, 3] replaced by the three JPEG keys."""
    fr = d["frames_u8"]
    T, n_img, H, W, _ = fr.shape
    if H % 16 or W % 16:
        raise ValueError(f"frames of {H} x {W}: the JPEG form needs sides that are multiples of 16 (resize or pad the frames first)")
    kw = dict(quality=int(quality), subsampling=SUBSAMPLING[subsampling])
    if restart_rows:
        kw["restart_marker_rows"] = int(restart_rows)
    files = []
    for img in fr.reshape(T * n_img, H, W, 3).numpy():
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", **kw)
        files.append(buf.getvalue())
    out = {k: v for k, v in d.items() if k != "frames_u8"}
    out["frames_jpeg"] = torch.from_numpy(np.frombuffer(b"".join(files), dtype=np.uint8).copy())
    out["frame_off"] = torch.from_numpy(np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64))
    out["frame_shape"] = torch.tensor([n_img, H, W], dtype=torch.int64)
    return out


def pack_on_device(d: dict, device: str, quality: int = 95, subsampling: str = "4:2:0", restart_rows: int = 1) -> dict:
    """pack() through the device's encoder: the same dict, its tensors on the host."""
    if subsampling != "4:2:0":
        raise ValueError(f"--device {device}: the device's encoder writes 4:2:0 only, got --subsampling {subsampling} (the Pillow path writes 4:4:4)")
    from vla_adapter_amd.jpeg_store import encode_tables
    out = encode_tables(d, device, int(quality), int(restart_rows), where="the source file")
    return {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--subsampling", choices=sorted(SUBSAMPLING), default="4:2:0")
    ap.add_argument("--restart_rows", type=int, default=1)
    ap.add_argument("--device", default="cpu", help="cpu: Pillow on the host (the default); cuda, cuda:0, ...: the device's encoder")
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    from vla_adapter_amd.episodes import _check_shard
    d = torch.load(args.src, weights_only=True, mmap=True)
    _check_shard(d, args.src)
    if "frames_u8" not in d:
        raise ValueError(f"{args.src}: already in the JPEG form")
    if args.device == "cpu":
        out = pack(d, args.quality, args.subsampling, args.restart_rows)
    else:
        out = pack_on_device(d, args.device, args.quality, args.subsampling, args.restart_rows)
    _check_shard(out, args.dst)
    torch.save(out, args.dst)
    raw, packed = int(d["frames_u8"].numel()), int(out["frames_jpeg"].numel())
    print(json.dumps(dict(src=args.src, dst=args.dst, frames=int(out["frame_off"].numel() - 1), quality=args.quality, subsampling=args.subsampling,
                          restart_rows=args.restart_rows, raw_bytes=raw, jpeg_bytes=packed, ratio=round(raw / packed, 3),
                          **({} if args.device == "cpu" else dict(device=args.device)))))


if __name__ == "__main__":
    main()
