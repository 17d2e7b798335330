#!/usr/bin/env python
"""The file codecs on splats that were not trained here: a .ply in, a compressed directory out, and back.

    python tools/ply_codec.py compress IN.ply DIR [--sort morton|grid|none] [--codec png|hevc] [--qp QP]
                                                                load_ply, then PngCompression / HevcCompression.compress
    python tools/ply_codec.py decompress DIR OUT.ply [--codec png|hevc]      the codec's decompress, then save_ply

A thin script over the APIs (gscodec_studio_amd.utils.load_ply / save_ply, gscodec_studio_amd.compression.PngCompression /
HevcCompression): the codec drops splats below its opacity threshold and crops to a square count, as it does for a trainer's splats.
``--codec hevc`` is the lossy one: ``--qp`` (0..51, default 4) trades bytes for quality.
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
    c.add_argument("--codec", choices=("png", "hevc"), default="png")
    c.add_argument("--qp", type=int, default=4, help="quantisation parameter of --codec hevc, 0..51")
    d = sub.add_parser("decompress")
    d.add_argument("dir")
    d.add_argument("ply")
    d.add_argument("--codec", choices=("png", "hevc"), default="png")
    args = ap.parse_args(argv)

    from gscodec_studio_amd.compression import HevcCompression, PngCompression
    from gscodec_studio_amd.utils import load_ply, save_ply

    if args.command == "compress":
        if not 0 <= args.qp <= 51:
            ap.error("--qp must lie in 0..51")
        sort = False if args.sort == "none" else args.sort
        codec = HevcCompression(use_sort=sort, verbose=False, qp=args.qp) if args.codec == "hevc" else PngCompression(use_sort=sort, verbose=False)
        splats = load_ply(args.ply)
        codec.compress(args.dir, dict(splats.items()))
        print(f"{args.ply}: {splats['means'].shape[0]} splats -> {args.dir}")
    else:
        codec = HevcCompression(verbose=False) if args.codec == "hevc" else PngCompression(verbose=False)
        splats = codec.decompress(args.dir)
        save_ply(splats, args.ply)
        print(f"{args.dir}: {splats['means'].shape[0]} splats -> {args.ply}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
