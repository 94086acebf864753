"""An ensemble of B member graphs against B single handles updated in turn
(DESIGN 8.6), in one process, after a warm-up of both forms, in interleaved
rounds.

  python tools/graph_members_probe.py [--rounds 5] [--parent-lib PATH] [--out FILE]
      [--shapes 72:1,16,64,256,1024 300:1,16,64,256] [--max-singles 256] [--singles-up-to 72:1024 300:16]

Shapes: 72 poses with 16 landmarks (circle_graph(72, n_landmarks=16, seed)) and
300 poses with 64 landmarks, both with their odometry edges; member k has seed k.
A round is one update of all members (wall clock around the call, which ends in
a synchronise) and one update of each single handle in turn.  Updates follow one
another from the current poses: the kernels' work does not depend on the poses.
Reported: ms per update of all members, member-updates per second, the ratio to
the single handles, min / median / max, and the per-phase device events of the
ensemble's last update.  At most --max-singles single handles are kept (each
owns two streams); a larger B updates them in turn several times over.  Beyond
--singles-up-to the single handles are not run ("not measured") and the ratio is
against B times the per-handle median of the largest B that was.

With --parent-lib (a libslam_hip.so of the parent commit, loaded through
SLAM_HIP_LIB in a fresh process, as this library is): the default path -- a plain
72-pose handle and the config-5 handle (50000 poses, PCG, cond="margin") -- in
interleaved rounds; this change's medians against the parent's spread, and the
PCG counts.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-robot_simu_amd"))

SIGMA = (0.02, 0.02, 0.01)
LANDMARKS = {72: 16, 300: 64}


def graph(T, seed):
    from slamhip.graph import circle_graph, circle_graph_odometry
    init, truth, edges = circle_graph(T, n_landmarks=LANDMARKS[T], seed=seed, odom_noise=0.002)
    return init, edges, circle_graph_odometry(truth, SIGMA, seed)


def stats3(v):
    return float(np.min(v)), float(np.median(v)), float(np.max(v))


def measure(T, B, rounds, max_singles, with_singles, say):
    from slamhip.graph import DeviceGraph, DeviceGraphEnsemble
    graphs = [graph(T, k % 64) for k in range(min(B, 64))]          # 64 distinct graphs, cycled
    ens = DeviceGraphEnsemble(solver="dense")
    ens.set_members([graphs[k % 64] for k in range(B)])
    singles = []
    if with_singles:
        for k in range(min(B, max_singles)):
            d = DeviceGraph(solver="dense")
            d.set_poses(graphs[k % 64][0])
            d.set_edges(graphs[k % 64][1], odometry=graphs[k % 64][2])
            singles.append(d)
    turns = (B + len(singles) - 1) // len(singles) if singles else 0

    solved = [B]                                                      # fewest members with is_calc = 1

    def run_ens():
        t0 = time.perf_counter()
        st = ens.update()
        ms = (time.perf_counter() - t0) * 1e3
        solved[0] = min(solved[0], int(np.sum(st[:, 0] == 1.0)))
        return ms

    def run_singles():
        t0 = time.perf_counter()
        n = 0
        for _ in range(turns):
            for d in singles:
                if n < B:
                    d.update()
                    n += 1
        return (time.perf_counter() - t0) * 1e3

    run_ens()                                                         # warm-up of both forms
    if singles:
        run_singles()
    e, s = [], []
    for _ in range(rounds):
        e.append(run_ens())
        if singles:
            s.append(run_singles())
    phases = ens._dev.timing()
    ens.close()
    for d in singles:
        d.close()
    if solved[0] != B:
        say("   (next row: only %d of %d members passed the gate in some update)" % (solved[0], B))
    return e, s, phases


def child_plain(args):
    """The default path of one library: a plain 72-pose handle, then config 5."""
    from slamhip.graph import DeviceGraph
    out = {}
    init, edges, odom = graph(72, 5)
    dev = DeviceGraph()
    dev.set_poses(init)
    dev.set_edges(edges, odometry=odom)
    dev.update()
    ms = []
    for _ in range(40):
        t0 = time.perf_counter()
        dev.update()
        ms.append((time.perf_counter() - t0) * 1e3)
    out["plain72_ms"] = float(np.median(ms))
    dev.close()
    g = np.load(args.graph)
    dev = DeviceGraph()                                               # config 5: PCG, cond="margin"
    dev.set_poses(g["init"])
    dev.set_edges(g["edges"])
    dev.update()
    ms, its = [], []
    for _ in range(3):
        dev.set_poses(g["init"])
        t0 = time.perf_counter()
        dev.update()
        ms.append((time.perf_counter() - t0) * 1e3)
        its.append(dev.timing()["pcg_iterations"])
    out["config5_ms"] = float(np.median(ms))
    out["config5_pcg"] = [int(i) for i in its]
    dev.close()
    print(json.dumps(out))


def run_child(graph_file, lib):
    env = dict(os.environ)
    if lib:
        env["SLAM_HIP_LIB"] = os.path.abspath(lib)
    else:
        env.pop("SLAM_HIP_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child-plain", "--graph", graph_file]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit("child failed (%d): nothing more is started" % r.returncode)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child-plain", action="store_true")
    ap.add_argument("--graph")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", nargs="*", default=["72:1,16,64,256,1024", "300:1,16,64,256"])
    ap.add_argument("--max-singles", type=int, default=256)
    ap.add_argument("--singles-up-to", nargs="*", default=["72:1024", "300:16"])
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_members_ab.txt"))
    args = ap.parse_args()
    if args.child_plain:
        return child_plain(args)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    upto = {int(a.split(":")[0]): int(a.split(":")[1]) for a in args.singles_up_to}
    say("ensemble of B members against B single handles updated in turn; one process, one warm-up of "
        "both forms, %d interleaved rounds; solver=\"dense\", odometry edges, wall clock in ms" % args.rounds)
    say()
    say("poses      B   ensemble min / median / max      singles min / median / max     "
        "member-updates/s   ratio (singles median / ensemble median)   ensemble phases of the last "
        "update (linearise, assemble, solve, pose update)")
    for shape in args.shapes:
        T = int(shape.split(":")[0])
        per_handle = None
        for B in [int(b) for b in shape.split(":")[1].split(",")]:
            with_singles = B <= upto.get(T, 0)
            e, s, ph = measure(T, B, args.rounds, args.max_singles, with_singles, say)
            emin, emed, emax = stats3(e)
            if with_singles:
                smin, smed, smax = stats3(s)
                per_handle = smed / B
                single_txt = "%9.3f %9.3f %9.3f" % (smin, smed, smax)
                ratio = "%.2f" % (smed / emed)
                if B > args.max_singles:
                    ratio += " (%d handles, %d turns)" % (args.max_singles, -(-B // args.max_singles))
                verdict = ""
                if B == 64 and T == 72:
                    verdict = "   [ensemble median %s the singles' minimum]" % (
                        "below" if emed < smin else "NOT below")
                if B == 1:
                    verdict = "   [ensemble median %s the single handle's spread; excess over its " \
                              "median %.3f ms]" % ("inside" if smin <= emed <= smax else "outside",
                                                   emed - smed)
            else:
                single_txt = "%29s" % "not measured"
                ratio = "not measured" if per_handle is None else \
                    "%.2f (against B x %.3f ms per handle, extrapolated)" % (B * per_handle / emed, per_handle)
                verdict = ""
            say("%5d %6d   %9.3f %9.3f %9.3f      %s   %14.0f   %s   %.3f %.3f %.3f %.3f%s" % (
                T, B, emin, emed, emax, single_txt, 1e3 * B / emed, ratio, ph["linearize_ms"],
                ph["assemble_ms"], ph["solve_ms"], ph["update_ms"], verdict))
    if args.parent_lib:
        from slamhip.graph import circle_graph
        say()
        say("the default path against the parent commit's library, interleaved rounds, a fresh process "
            "each: a plain 72-pose handle (median of 40 updates) and config 5 (50000 poses, PCG, "
            "cond=\"margin\"; median of 3 updates from the initial poses)")
        say("round   parent plain72 ms   this plain72 ms   parent config5 ms   this config5 ms   PCG counts")
        with tempfile.TemporaryDirectory() as tmp:
            gf = os.path.join(tmp, "c5.npz")
            init, _, edges = circle_graph(50000, n_landmarks=64, seed=0, odom_noise=0.002)
            np.savez(gf, init=init, edges=edges)
            par, new = [], []
            for i in range(args.rounds):
                p, n = run_child(gf, args.parent_lib), run_child(gf, None)
                par.append(p)
                new.append(n)
                say("%5d %19.3f %17.3f %19.3f %17.3f   %s / %s" % (
                    i, p["plain72_ms"], n["plain72_ms"], p["config5_ms"], n["config5_ms"],
                    p["config5_pcg"], n["config5_pcg"]))
        for key in ("plain72_ms", "config5_ms"):
            pv, nv = [p[key] for p in par], [n[key] for n in new]
            med = float(np.median(nv))
            say("%s: parent min %.3f median %.3f max %.3f; this min %.3f median %.3f max %.3f; this "
                "median %s the parent's spread" % (key, *stats3(pv), *stats3(nv),
                                                   "lies inside" if min(pv) <= med <= max(pv) else
                                                   ("lies BELOW" if med < min(pv) else "lies ABOVE")))
        say("PCG counts equal: %s" % all(p["config5_pcg"] == n["config5_pcg"] for p, n in zip(par, new)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
