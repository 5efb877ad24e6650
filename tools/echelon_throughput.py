"""Throughput of the echelon general kernel (cpecan_k_generale): one batch of synthetic reads, banded, posterior
decode; prints the kernel time and Gcells/s (in-band cells / kernel time) as one JSON line.  Informational.

    python tools/echelon_throughput.py [--reads 1024] [--lx 400] [--ly 800] [--expansion 100] [--runs 3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

import synth  # noqa: E402
from cpecan_load import binding  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1024)
    ap.add_argument("--lx", type=int, default=400)
    ap.add_argument("--ly", type=int, default=800)
    ap.add_argument("--expansion", type=int, default=100)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    cp = binding()
    ctx = cp.Context(0)
    batch = synth.make_batch(7, a.reads, a.lx, a.ly, anchor_every=50)
    rng = np.random.default_rng(7)
    batch["events"][:, 2] = rng.uniform(0.0008, 0.012, batch["events"].shape[0])
    models = []
    for match, _, gap_y in batch["models"]:
        skip = np.sort(rng.uniform(0.05, 0.4, 30))[::-1]
        models.append(((0.79015888282447311, 0.19652425498269727), match, np.concatenate([skip, skip]), gap_y))
    ids = ctx.modelse_create(models)
    items = np.zeros(len(batch["items"]), cp.ITEM_DTYPE)
    for i, it in enumerate(batch["items"]):
        items[i] = (it["x_offset"], it["lX"], it["y_offset"], it["lY"], it["anchor_offset"], it["n_anchors"],
                    ids[it["model"]], 1, 1, 0)
    bp = cp.BandParams(0.01, 1000, 40, a.expansion)
    b = cp.Batch(ctx, items, batch["x_chars"], batch["events"], batch["anchors"], bp, echelon=True)
    times = []
    for _ in range(a.runs + 1):
        b.run()
        b.sync()
        times.append(b.elapsed_ms()[1])
    cells = int(b.counts()[2].sum())
    ms = float(np.median(times[1:]))
    print(json.dumps(dict(kernel="cpecan_k_generale", reads=a.reads, lX=a.lx, lY=a.ly, expansion=a.expansion,
                          cells=cells, kernel_ms=round(ms, 3), gcells_per_s=round(cells / ms / 1e6, 3),
                          info=b.info())))
    b.close()
    ctx.close()


if __name__ == "__main__":
    main()
