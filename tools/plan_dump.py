#!/usr/bin/env python3
"""Dumps the dispatcher's decisions over a fixed grid, one line per point, so that two builds of the library can be `diff`ed after a
planner change (pure host logic: no GPU).  QQQ_AMD_LIB selects the build, as everywhere.

    python tools/plan_dump.py > new.txt;  QQQ_AMD_LIB=/path/to/old/libqqq_amd.so python tools/plan_dump.py > old.txt;  diff old.txt new.txt
    python tools/plan_dump.py 3/8      # shard 3 of 8 (the layer shapes are dealt round-robin): run the shards side by side

A line: M N K groupsize max_par have_scratch have_workspace tune | rc and the 14 fields of qqq_w4a8_plan | rc and the four doubles of
qqq_w4a8_model_us (float.hex).  The grid: every layer shape of the committed dispatch-check files, the six of
test_dispatch_plan_respects_scratch_contract, (64, 128), K % 128 == 64 and packed weights >= 4 GiB; M = 1 ... 1100, every 37th to 70000, the
multiples of 256 up to 9216 and their neighbours; both modes; max_par 0 / 1 / 4 / 8 / 16; with and without C / workspace; no tune and
each family forced -- plus 20000 random qqq_tune_t (documented values and some outside them) on the dispatch-check shapes."""
import ctypes
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qqq_amd import _lib  # noqa: E402
from tools import dispatch_regret  # noqa: E402

FIELDS = [f for f, _ in _lib.QQQTune._fields_]
RANDOM = dict(kernel=range(7), ksplit=(-1, 0, 1, 2, 3, 4, 8, 300), waves=(0, 4, 5, 8, 16), fused=range(256), bm=(0, 64, 100, 128, 130, 131, 256, 258, 259),
              glds=range(3), pf=(0, 2, 3, 4, 5, 7, 8, 12), stages=range(9), mt=(0, 1, 2, 3, 4, 8, 16), pw=(0, 1, 2, 4, 8, 16, 32), nslots=(0,),
              split_m=(-1, 0), skew=(-1, 0, 5, 100), w8=(-1, 0, 1))


def main():
    shard, nshards = (int(v) for v in sys.argv[1].split("/")) if len(sys.argv) > 1 else (0, 1)
    L = _lib.lib()
    checked = sorted({(int(m.group(1)), int(m.group(2))) for f in dispatch_regret.grid_files() for m in map(dispatch_regret.LINE.match, open(f)) if m})
    extra = [(8192, 21760), (4096, 4096), (11008, 4096), (4096, 11008), (256, 128), (320, 1536), (64, 128), (4096, 4160), (65536, 131072)]
    shapes = checked + [s for s in extra if s not in checked]
    ms = sorted(set(range(1, 1101)) | set(range(1137, 70001, 37)) | {m + d for m in range(256, 9217, 256) for d in (-1, 0, 1)})
    out, us = _lib.QQQTune(), (ctypes.c_double * 4)()
    write = sys.stdout.write

    def point(m, n, k, gs, mp, hs, hw, tune, label, model):
        rc = L.qqq_w4a8_plan(m, n, k, gs, mp, hs, hw, ctypes.byref(tune) if tune is not None else None, ctypes.byref(out))
        write(f"{m} {n} {k} {gs} {mp} {hs} {hw} {label} | {rc} {' '.join(str(getattr(out, f)) for f in FIELDS)} | {model}\n")

    def model(m, n, k, gs, mp):
        rc = L.qqq_w4a8_model_us(m, n, k, gs, mp, us)
        return f"{rc} {' '.join(float(v).hex() for v in us)}"

    forced = [(None, "auto")] + [(_lib.QQQTune(kernel=kern), f"kernel={kern}") for kern in range(1, 6)]
    for n, k in shapes[shard::nshards]:
        for m in ms:
            for gs in (-1, 128):
                for mp in (0, 1, 4, 8, 16):
                    price = model(m, n, k, gs, mp)
                    for hs in (0, 1):
                        for hw in (0, 1):
                            for tune, label in forced:
                                point(m, n, k, gs, mp, hs, hw, tune, label, price)
    rng = random.Random(0)
    for i in range(20000):
        tune = _lib.QQQTune(**{f: rng.choice(RANDOM[f]) for f in FIELDS})
        gs, mp, hs, hw = rng.choice((-1, 128)), rng.choice((0, 1, 4, 8, 16)), rng.randrange(2), rng.randrange(2)
        label = "tune=" + ",".join(str(getattr(tune, f)) for f in FIELDS)
        for n, k in checked[shard::nshards]:
            for m in (1, 16, 64, 128, 300, 1024, 4097):
                point(m, n, k, gs, mp, hs, hw, tune, label, model(m, n, k, gs, mp))


if __name__ == "__main__":
    main()
