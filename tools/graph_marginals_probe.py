"""slam_graph_marginals on the config-5 graph: time per call, per pass-iteration
and per column at every pass width, against the single-right-hand-side PCG
iteration of update() measured in the same process (development probe; writes
profiles/graph_marginals_ab.txt).

One process, circle_graph(50000, n_landmarks=64, seed=3, odom_noise=0.002)
after optimize().  Every (m, width) shape is warmed once, then the shapes run
alternately, nine rounds; the call's time is the C-ABI's own device-event
figure (info[4]), the median over the rounds.  Bytes per pass-iteration are
counted from shapes: every 3x3 block and its column index once (n_slots x 80
B), the block-Jacobi inverses once (9 n_t x 8 B), and per column twelve vector
passes of n doubles (SpMM: z gathered, p and q read and written, z own rows;
step: x and r read and written, p, q read, z written).

Both fold forms are timed: every workgroup folding the scalar partials
redundantly (the default) and a one-workgroup fold launch before each of the
two kernels (SLAM_GRAPH_MARG_FOLD=1; the same bits).  An argument names another
output file.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-robot_simu_amd"))
from slamhip.graph import DeviceGraph, circle_graph  # noqa: E402

N_POSES = int(os.environ.get("MARG_PROBE_POSES", "50000"))
WIDTHS = (1, 2, 4, 8)
MS = (1, 8, 64)
ROUNDS = 9


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles",
                                                                  "graph_marginals_ab.txt")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    init, _, edges = circle_graph(N_POSES, n_landmarks=64, seed=3, odom_noise=0.002)
    # the yardstick: update()'s own PCG, without the cond estimate beside it
    dev = DeviceGraph(solver="pcg", pcg_tol=1e-10, cond="off")
    dev.set_poses(init)
    dev.set_edges(edges)
    st = dev.optimize(0.01, 20)
    say(f"graph: {N_POSES} poses, {len(edges)} edges; optimize: {len(st)} iterations, "
        f"last sum delta^2 {st[-1][1]:.3e}")
    single = []
    for _ in range(5):
        dev.update()
        t = dev.timing()
        single.append((t["solve_ms"], t["pcg_iterations"]))
    s_ms, s_it = np.median([a for a, _ in single]), int(np.median([b for _, b in single]))
    us_single = 1e3 * s_ms / s_it
    say(f"single right-hand side (update(), cond off): solve {s_ms:.3f} ms / {s_it} iterations = "
        f"{us_single:.2f} us per iteration")
    rows, _, _ = dev.get_bsr()
    n_slots, nt = len(rows), len(dev.get_system(dense=False)[0])
    n = 3 * nt
    say(f"H: {n_slots} blocks ({n_slots * 80 / 1e6:.1f} MB with column indices), n = {n}")

    shapes = [(m, w, fold) for m in MS for w in WIDTHS for fold in ("redundant", "launch")]
    times = {m: np.linspace(0, nt - 1, m).astype(np.int64) if m > 1 else np.array([nt - 1])
             for m in MS}
    res = {s: [] for s in shapes}
    info = {}
    for rnd in range(ROUNDS + 1):                     # round 0 warms every shape
        for m, w, fold in shapes:
            dev.set_marginal_cols(w)
            os.environ["SLAM_GRAPH_MARG_FOLD"] = "1" if fold == "launch" else "0"
            ok, _, inf = dev.marginals(times[m], relinearize=False)
            assert ok, (m, w, fold, inf)
            if rnd:
                res[(m, w, fold)].append(inf["ms"])
            info[(m, w, fold)] = inf
    os.environ.pop("SLAM_GRAPH_MARG_FOLD", None)
    say()
    say("   m  cols  folds      passes  max it   call ms   us/pass-it   x single   us/col-it   GB/s (counted)")
    for m, w, fold in shapes:
        inf = info[(m, w, fold)]
        ms = float(np.median(res[(m, w, fold)]))
        # every pass runs to its slowest column; max it bounds the passes' lengths
        pass_its = inf["passes"] * inf["iterations"]
        us_pi = 1e3 * ms / pass_its
        width = min(w, min(x for x in WIDTHS if x >= min(3 * m, w)))    # a narrow request runs narrower
        byts = n_slots * 80 + 9 * nt * 8 + width * 12 * n * 8
        say(f"{m:4d} {w:5d}  {fold:9s} {inf['passes']:7d} {inf['iterations']:7d} {ms:9.3f} {us_pi:12.2f} "
            f"{us_pi / us_single:10.2f} {us_pi / width:11.2f} {byts / (us_pi * 1e-6) / 1e9:10.1f}")
    say()
    say("us/pass-it: call ms / (passes x max iterations of a column), an upper bound on the passes' "
        "work since only the slowest pass runs that long; x single: against the single-RHS iteration "
        "above; a pass narrower than cols runs at the smallest width that holds it.")
    dev.close()
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
