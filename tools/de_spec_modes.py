"""Forced store modes of the chained DE kernel (sx_de_args.spec_store) at chosen generations of the headline run:
python tools/de_spec_modes.py [n P [reps]] -> one line per (start generation, window): us per generation for spec_store =
1 (late), 2 (trial-early), 3 (old-early), 0 (trial early + winner late: what runs), and the win fraction of the window's
generations.

The run is brought to the start generation, its device state is saved, and a K-generation graph is replayed `reps` times
from that state (restored by device copies in front of the start event), timed by HIP events; the median counts.  The
restoring copies leave the population in a cache state of their own, the same for every mode: compare the columns of a line
with each other, not with bench.py."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch
from stochopy_amd import _lib
from stochopy_amd.optimize import _de

n, P = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (128, 4096)
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 200
WINDOWS = [(3, 2), (5, 2), (7, 2), (9, 2), (12, 2), (14, 2), (22, 2), (66, 2), (66, 20), (3000, 2), (3000, 20)]


def one(mode, g0, K):
    run = _de._DeRun(_lib.FUN_IDS["rosenbrock"], np.full(n, -5.12), np.full(n, 5.12), None, 2**31 - 2, P, 0.5, 0.9, "best1bin",
                     None, 0.0, -1.0, False, 1.0, None, "philox", 1234, 1, autorun=False, spec_store=mode)
    ctx = run.ctx
    try:
        with torch.cuda.stream(ctx.stream):
            run._setup()
            run.enqueue(g0 - 1)  # the population now holds generation g0
            par = run.launches & 1
            graph = run._chain_graph(par, K)
            live = [run.bufs[0], run.bufs[1], run.fit, run.candfit, run.state, run.part_f, run.part_i]
            saved = [t.clone() for t in live]
            wins = []
            for _ in range(K):  # win fractions of the window (and a first, untimed pass over it)
                f0 = run.fit.clone()
                run._chain_launch(run.launches & 1, 0)
                run.launches += 1
                ctx.sync()
                wins.append(float((run.fit != f0).double().mean()))
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
            for e0, e1 in ev:
                for t, s in zip(live, saved):
                    t.copy_(s)
                e0.record(ctx.stream)
                _lib.check(ctx.L.sx_graph_launch(graph, ctx.stream_ptr), "sx_graph_launch")
                e1.record(ctx.stream)
            ctx.sync()
            us = np.array([e0.elapsed_time(e1) for e0, e1 in ev][reps // 10:]) * 1e3 / K
            check = float(run.fit.sum())
    finally:
        run.close()
    return float(np.median(us)), float(np.percentile(us, 10)), float(np.percentile(us, 90)), wins, check


print("n %d P %d, %d replays per cell (first tenth dropped): median us per generation [10th .. 90th percentile]" % (n, P, reps))
for g0, K in WINDOWS:
    cells, wins, checks = [], None, set()
    for mode in (1, 2, 3, 0):
        med, lo, hi, wins, check = one(mode, g0, K)
        cells.append("%d: %.3f [%.3f .. %.3f]" % (mode, med, lo, hi))
        checks.add(check)
    print("generations %5d..%-5d win %.2f (%s)  %s  %s" % (g0 + 1, g0 + K, float(np.mean(wins)),
                                                         " ".join("%.2f" % w for w in wins[:4]), "   ".join(cells),
                                                         "same fit" if len(checks) == 1 else "FIT DIFFERS"), flush=True)
