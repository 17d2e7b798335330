#!/usr/bin/env python
"""The PNG codec on splats that were not trained here: a .ply in, a compressed directory out, and back.

    python tools/ply_codec.py compress IN.ply DIR [--sort morton|grid|none]     load_ply, then PngCompression.compress
    python tools/ply_codec.py decompress DIR OUT.ply                             PngCompression.decompress, then save_ply

A thin script over the two APIs (gscodec_studio_amd.utils.load_ply / save_ply, gscodec_studio_amd.compression.PngCompression):
the codec drops splats below its opacity threshold and crops to a square count, as it does for a trainer's splats.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)
    c = sub.add_parser("compress")
    c.add_argument("ply")
    c.add_argument("dir")
    c.add_argument("--sort", choices=("morton", "grid", "none"), default="morton")
    d = sub.add_parser("decompress")
    d.add_argument("dir")
    d.add_argument("ply")
    args = ap.parse_args(argv)

    from gscodec_studio_amd.compression import PngCompression
    from gscodec_studio_amd.utils import load_ply, save_ply

    if args.command == "compress":
        splats = load_ply(args.ply)
        PngCompression(use_sort=False if args.sort == "none" else args.sort, verbose=False).compress(args.dir, dict(splats.items()))
        print(f"{args.ply}: {splats['means'].shape[0]} splats -> {args.dir}")
    else:
        splats = PngCompression(verbose=False).decompress(args.dir)
        save_ply(splats, args.ply)
        print(f"{args.dir}: {splats['means'].shape[0]} splats -> {args.ply}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
