#!/usr/bin/env python3
"""Run PredNet over a short video on the MI355X engine and write what it predicts, with the flow between predictions.

    python examples/predict_sequence.py -o seq_out [-i frames_dir] [-m model.npz] [--size 160x120] [-c 3] [--ext 2]

Input: the PNG files of a folder, in name order, centre-cropped to --size; without -i, a drifting synthetic pattern.
Output: pred_NNN.png (the prediction after frame NNN; the last --ext are fed their own prediction) and flow_NNN.png
(Lucas-Kanade vectors between predictions NNN and NNN + 1, drawn 20x over prediction NNN).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
from PIL import Image, ImageDraw

from evolutionary_illusion_generator_amd import fitness


def read_frames(folder, c_dim, w, h):
    names = sorted(f for f in os.listdir(folder) if f.lower().endswith(".png"))
    if not names:
        raise SystemExit("no PNG files in %s" % folder)
    return np.stack([fitness._read_image_chw(os.path.join(folder, f), c_dim, w, h) for f in names])


def drifting_pattern(n, c_dim, w, h):
    """Concentric rings drifting one pixel right and half a pixel down per frame."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    frames = []
    for t in range(n):
        r = np.hypot(xx - w / 2 - t, yy - h / 2 - 0.5 * t)
        v = 127.5 + 127.5 * np.sin(r / 3.0)
        frames.append(np.repeat(v[None], c_dim, axis=0).astype(np.uint8))
    return np.stack(frames)


def to_pil(chw):
    return Image.fromarray(chw[0] if chw.shape[0] == 1 else chw.transpose(1, 2, 0))


def overlay(chw, vectors, scale=20.0):
    im = to_pil(chw).convert("RGB")
    d = ImageDraw.Draw(im)
    for x, y, dx, dy in vectors:
        d.line([(x, y), (x + scale * dx, y + scale * dy)], fill=(255, 0, 0), width=1)
        d.ellipse([x - 1, y - 1, x + 1, y + 1], fill=(255, 255, 0))
    return im


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", "-i", default=None, help="folder of PNG frames (default: a drifting synthetic pattern)")
    ap.add_argument("--output_dir", "-o", default="seq_out")
    ap.add_argument("--model", "-m", default="synthetic", help="chainer npz weights, or synthetic[:seed]")
    ap.add_argument("--size", default="160x120", help="WxH")
    ap.add_argument("--color_space", "-c", type=int, default=3)
    ap.add_argument("--channels", "-ch", default=None, help="PredNet channels (default: c,48,96,192)")
    ap.add_argument("--frames", type=int, default=12, help="synthetic frames (without -i)")
    ap.add_argument("--ext", type=int, default=2, help="self-fed steps after the last frame")
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.lower().split("x"))
    channels = [int(c) for c in args.channels.split(",")] if args.channels else [args.color_space, 48, 96, 192]
    c_dim = channels[0]
    frames = read_frames(args.input, c_dim, w, h) if args.input else drifting_pattern(args.frames, c_dim, w, h)
    preds = fitness.prednet_sequence_predictions(frames[None], args.model, channels, w, h, n_ext=args.ext)[0]
    flows = fitness.sequence_flow(preds[None])[0]
    os.makedirs(args.output_dir, exist_ok=True)
    for t, p in enumerate(preds):
        to_pil(p).save(os.path.join(args.output_dir, "pred_%03d.png" % t))
    for t, v in enumerate(flows):
        overlay(preds[t], v).save(os.path.join(args.output_dir, "flow_%03d.png" % t))
    print("%d frames -> %d predictions, %d flow overlays in %s (vectors per pair: %s)"
          % (len(frames), len(preds), len(flows), args.output_dir, [len(v) for v in flows]))


if __name__ == "__main__":
    main()
