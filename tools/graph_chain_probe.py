"""Cost and gain of the chain preconditioner at the config-5 shape:
circle_graph(50000, n_landmarks=64, seed=0, odom_noise=0.002) without and with
circle_graph_odometry(truth, (0.02, 0.02, 0.01), 0), PCG path (pcg_tol 1e-10),
cond="estimate".

  python tools/graph_chain_probe.py [--parent-lib PATH] [--rounds 5] [--out FILE]

One fresh process per row: block-Jacobi and chain S in {1, 4, 16, 64}, each
without and with the odometry edges; every update from the initial poses after
one warm-up, medians.  "us / it" is the solve time between the handle's events
over the PCG iterations: both launches of an iteration, with the factor, the
start kernel and the host's polls spread over them.  The factor's own time is
the difference of two timed apply_precond calls, the first of which factors
(wall clock, so it carries the launch; a kernel trace gives the kernel alone).

With --parent-lib (a libslam_hip.so built from the parent commit, loaded
through SLAM_HIP_LIB): the default path (no odometry, cond="margin") against it
in interleaved rounds, this change's median update inside the parent's spread;
and the parent's block-Jacobi row with odometry edges re-measured the same way,
whose minimum update the chain S = 64 row has to beat.
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


def make_graph():
    from slamhip.graph import circle_graph, circle_graph_odometry
    init, truth, edges = circle_graph(50000, n_landmarks=64, seed=0, odom_noise=0.002)
    return init, edges, circle_graph_odometry(truth, SIGMA, 0)


def child(args):
    from slamhip.graph import DeviceGraph
    if args.graph:
        g = np.load(args.graph)
        init, edges, odom = g["init"], g["edges"], g["odom"]
    else:
        init, edges, odom = make_graph()
    dev = DeviceGraph(solver="pcg", pcg_tol=1e-10, cond=args.cond)
    chain = args.segment >= 0
    if chain:
        dev.set_precond("chain", args.segment)
    dev.set_poses(init)
    if args.odom:
        dev.set_edges(edges, odometry=odom)
    else:
        dev.set_edges(edges)                       # the call a parent library has
    dev.update()                                   # warm-up (cold cond estimate, allocations)
    upd, sol, its, calc = [], [], [], True
    for _ in range(args.updates):
        dev.set_poses(init)
        t0 = time.perf_counter()
        st = dev.update()
        upd.append((time.perf_counter() - t0) * 1e3)
        t = dev.timing()
        sol.append(t["solve_ms"])
        its.append(t["pcg_iterations"])
        calc = calc and st[0]
    out = dict(odom=int(args.odom), segment=args.segment, is_calc=bool(calc),
               update_ms=float(np.median(upd)), update_min_ms=float(np.min(upd)),
               update_max_ms=float(np.max(upd)), solve_ms=float(np.median(sol)),
               pcg_iterations=int(np.median(its)), cond=float(st[3]), edges=int(dev.n_edges))
    if hasattr(dev._lib, "slam_graph_apply_precond"):
        r = np.ones(3 * 50000)
        fac, app = [], []
        for _ in range(5):
            dev.marginals([7], relinearize=True)   # a new assembly: the next apply factors
            t0 = time.perf_counter()
            dev.apply_precond(r)
            t1 = time.perf_counter()
            dev.apply_precond(r)
            t2 = time.perf_counter()
            fac.append(((t1 - t0) - (t2 - t1)) * 1e3)
            app.append((t2 - t1) * 1e3)
        out.update(factor_ms=float(np.median(fac)), apply_call_ms=float(np.median(app)),
                   info=dev.precond_info())
    dev.close()
    print(json.dumps(out))


def run_child(graph, odom, segment, args, lib=None, cond="estimate"):
    env = dict(os.environ)
    if lib:
        env["SLAM_HIP_LIB"] = os.path.abspath(lib)
    else:
        env.pop("SLAM_HIP_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--graph", graph, "--odom", str(int(odom)),
           "--segment", str(segment), "--updates", str(args.updates), "--cond", cond]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit("child failed (%d): nothing more is started" % r.returncode)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--graph")
    ap.add_argument("--odom", type=int, default=0)
    ap.add_argument("--segment", type=int, default=-1, help="-1: block-Jacobi")
    ap.add_argument("--updates", type=int, default=7)
    ap.add_argument("--cond", default="estimate")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_chain_ab.txt"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    init, edges, odom = make_graph()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    with tempfile.TemporaryDirectory() as tmp:
        graph = os.path.join(tmp, "c5.npz")
        np.savez(graph, init=init, edges=edges, odom=odom)
        say("graph: 50000 poses, %d pair edges, %d odometry edges (sigma %g %g %g), PCG path (pcg_tol "
            "1e-10), cond=\"estimate\"; %d updates per process after one warm-up, every one from the "
            "initial poses, medians" % (len(edges), len(odom), *SIGMA, args.updates))
        say()
        say("odometry   preconditioner   PCG it   solve ms   us / it   update ms (wall)   update min   "
            "factor ms (wall)   apply call ms   off-diagonal blocks   bad pivots")
        rows = {}
        for od in (0, 1):
            for seg in (-1, 1, 4, 16, 64):
                r = rows[od, seg] = run_child(graph, od, seg, args)
                say("%-10s %-16s %6d %10.3f %9.2f %18.3f %12.3f %18.4f %15.4f %21d %12d%s" % (
                    "yes" if od else "no", "block-Jacobi" if seg < 0 else "chain S=%d" % seg,
                    r["pcg_iterations"], r["solve_ms"], 1e3 * r["solve_ms"] / max(r["pcg_iterations"], 1),
                    r["update_ms"], r["update_min_ms"], r["factor_ms"], r["apply_call_ms"],
                    r["info"]["off_diagonal_blocks"], r["info"]["bad_pivots"],
                    "" if r["is_calc"] else "   (is_calc = 0)"))
        if args.parent_lib:
            for od, cond, what in ((0, "margin", "default path (no odometry edges, cond=\"margin\")"),
                                   (1, "estimate", "block-Jacobi with odometry edges (cond=\"estimate\")")):
                say()
                say("%s against the parent commit's library, interleaved rounds (a fresh process each):" % what)
                say("round   parent update ms   parent PCG it   this update ms   this PCG it")
                par, new = [], []
                for i in range(args.rounds):
                    p = run_child(graph, od, -1, args, lib=args.parent_lib, cond=cond)
                    n = run_child(graph, od, -1, args, cond=cond)
                    par.append(p)
                    new.append(n)
                    say("%5d %18.3f %15d %16.3f %13d" % (i, p["update_ms"], p["pcg_iterations"],
                                                       n["update_ms"], n["pcg_iterations"]))
                pu = [p["update_ms"] for p in par]
                nu = [n["update_ms"] for n in new]
                med = float(np.median(nu))
                say("parent update ms: min %.3f median %.3f max %.3f; this: min %.3f median %.3f max %.3f" % (
                    min(pu), float(np.median(pu)), max(pu), min(nu), med, max(nu)))
                say("this median %s the parent's spread [%.3f, %.3f]" % (
                    "lies inside" if min(pu) <= med <= max(pu) else
                    ("lies BELOW" if med < min(pu) else "lies ABOVE"), min(pu), max(pu)))
                assert all(p["pcg_iterations"] == n["pcg_iterations"] for p, n in zip(par, new))
                if od:
                    floor = min(p["update_min_ms"] for p in par)
                    for seg in (1, 4, 16, 64):
                        u = rows[1, seg]["update_ms"]
                        say("chain S=%d update %.3f ms %s the minimum of the parent's block-Jacobi updates "
                            "(%.3f ms)" % (seg, u, "is below" if u < floor else "is NOT below", floor))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
