#!/usr/bin/env python3
"""Distinct cache lines per deep gather of the ring walk, priced on the host for every placement of the super-node
groups ("ohx_super_pack" 0..3, csrc/flatten.hpp): the table of profiles/r12_line_count.txt, docs/04 section 4.13.

The benchmark booster (100 trees, depth 18) and the sample profiles/r05_sweeps.txt used: 300 bricks of 4 x 4 x 4
gridcells spread over the lower 52 levels of the C360 batch (tests/analysis/quad_lookups.py draws the same ones).  That
file predicted 39.1 tag look-ups per gather for the shipped lane order against 38.4 measured
(TCP_TOTAL_CACHE_ACCESSES per vector-memory instruction); the look-ups this counter reports for super_pack 0 on the same
bricks are its calibration.  The lines of a BLOCK need neighbours, so every brick is also counted together with the 15
tiles that share its block of 16 in launch order (tiles are numbered brick-i fastest, walk_device.hpp tile_row).

The counting is native (csrc/line_count.cpp) and walks with the host walk of the layout tests (csrc/super_walk.hpp).
usage: python3 tools/line_count.py [--bricks 300] [--trees 100] [--depth 18]      (CPU only, about a minute)"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quickchem_amd import synth  # noqa: E402

NAMES = {0: "breadth first (parent)", 1: "+ 128-byte tree bases", 2: "+ sibling pairs", 3: "+ families"}


def brick_rows(grid, bi, bj, bk):
    """(64, 27): the gridcells of brick (bi, bj, bk) of 4 x 4 x 4 in grid order, i fastest"""
    im, jm, _ = grid
    out = np.empty((4, 4, 4, synth.NFEAT), dtype=np.float32)
    for kk in range(4):
        for jj in range(4):
            out[kk, jj] = synth.rows_cpu(grid, 4 * bi + im * ((4 * bj + jj) + jm * (4 * bk + kk)), 4)
    return out.reshape(64, synth.NFEAT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bricks", type=int, default=300)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--depth", type=int, default=18)
    ap.add_argument("--grid", default="C360")
    args = ap.parse_args()
    t0 = time.time()
    model = synth.make_model(num_trees=args.trees, max_depth=args.depth, sample_log2=20)
    grid = synth.GRIDS[args.grid]
    im, jm, km = grid
    nbi, nbj = im // 4, jm // 4
    rng = np.random.default_rng(1)
    picked = []
    for _ in range(args.bricks):      # the draws of tests/analysis/quad_lookups.py, in its order
        bi = int(rng.integers(0, im // 4)); bj = int(rng.integers(0, jm // 4)); bk = int(rng.integers(5, km // 4))
        picked.append((bi, bj, bk))
    alone = np.stack([brick_rows(grid, *b) for b in picked])
    blocks = []
    for bi, bj, bk in picked:
        first = (bi + nbi * (bj + nbj * bk)) // 16 * 16
        for t in range(first, first + 16):
            blocks.append(brick_rows(grid, t % nbi, (t // nbi) % nbj, t // (nbi * nbj)))
    blocks = np.stack(blocks)
    print(f"# python3 tools/line_count.py --bricks {args.bricks} --trees {args.trees} --depth {args.depth} --grid {args.grid}")
    print(f"# booster: {model.num_trees} trees, {model.num_nodes} nodes; {args.bricks} bricks of 4 x 4 x 4, k fastest among the "
          f"lanes; their blocks: {blocks.shape[0]} tiles   (inputs in {time.time() - t0:.0f} s)")
    print("# per wave-gather of the steps the ring kernels fetch from memory (step 5 = the fifth super-node of a walk):")
    print("#   records = distinct 16-byte records among the 64 lanes; look-ups = distinct 64-byte blocks per quad, summed")
    print("#   over the 16 quads; lines = distinct 128-byte lines among the 64 lanes; block lines = distinct 128-byte lines")
    print("#   among the 16 tiles of a block (same tree, same step)")
    base_records = None
    for pack in synth.SUPER_PACKS:
        t1 = time.time()
        one, info = synth.super_line_count(model.image, alone, pack, brick=(2, 2, 2), k_fastest=True)
        blk, _ = synth.super_line_count(model.image, blocks, pack, brick=(2, 2, 2), k_fastest=True)
        if base_records is None:
            base_records = info["records"]
        print(f"\nohx_super_pack={pack}  {NAMES[pack]}: {info['records']} records ({info['records'] * 16 / 2**20:.2f} MiB, "
              f"{100.0 * (info['records'] - base_records) / base_records:+.3f} % against 0), {info['fillers']} fillers, "
              f"{info['packed_trees']} of {model.num_trees} trees numbered by line   ({time.time() - t1:.0f} s)")
        print("  step  gathers   records  look-ups     lines | in their blocks: look-ups     lines  block lines  per tile")
        tot = np.zeros(6)
        n = nb = 0
        for s in sorted(one):
            a, b = one[s], blk[s]
            print(f"  {s + 1:4d} {a['gathers']:8d}  {a['records']:8.2f}  {a['lookups']:8.2f}  {a['lines']:8.2f} |"
                  f"                  {b['lookups']:8.2f}  {b['lines']:8.2f}     {b['block_lines']:8.1f}  {b['block_lines'] / 16:8.2f}")
            tot += np.array([a['records'], a['lookups'], a['lines'], b['lookups'], b['lines'], b['block_lines']]) * np.array(
                [a['gathers']] * 3 + [b['gathers']] * 3)
            n += a['gathers']; nb += b['gathers']
        print(f"   all {n:8d}  {tot[0] / n:8.2f}  {tot[1] / n:8.2f}  {tot[2] / n:8.2f} |"
              f"                  {tot[3] / nb:8.2f}  {tot[4] / nb:8.2f}     {tot[5] / nb:8.1f}  {tot[5] / nb / 16:8.2f}")


if __name__ == "__main__":
    main()
