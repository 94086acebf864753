"""Cost of the odometry edges at the config-5 shape:
circle_graph(50000, n_landmarks=64, seed=0, odom_noise=0.002) with
circle_graph_odometry(truth, (0.02, 0.02, 0.01), 0): 199,979 pair edges and
49,999 odometry edges, PCG path, cond="estimate".

  python tools/graph_odom_probe.py [--parent-lib PATH] [--rounds 5] [--out FILE]

One child process without and one with the odometry edges: the structure build
(set_edges, wall clock, median of `--builds` calls), the linearise time between
the handle's two events, the assembly, the update (wall clock), the PCG
iteration count and the time of a chi2() call, each update from the initial
poses.  The two linearise launches are each timed alone between those events: the
landmark launch in the child without odometry edges, the odometry launch in a
third child whose edge set holds the 49,999 odometry edges and no pair (its
columns have stride 49,999, not 249,978; its solve is cut short at 50 PCG
iterations, only the linearise time is read).  The child with both kinds has
both launches between the events.  Nothing here is a prediction: the file
records what was found.

With --parent-lib (a libslam_hip.so built from the parent commit, loaded
through SLAM_HIP_LIB) the default path -- no odometry, the default gate -- is
measured against it in interleaved rounds, one fresh process per library and
round; this change's median update time must lie inside the spread (min .. max)
of the parent's own rounds.
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


def child(args):
    from slamhip.graph import DeviceGraph
    g = np.load(args.graph)
    init, edges = g["init"], g["edges"]
    odom = g["odom"] if args.odom else None
    if args.odom == 2:                             # the odometry launch alone
        edges = edges[:0]
        dev = DeviceGraph(solver="pcg", pcg_tol=1e-10, cond="off", pcg_max_iter=50)
    else:
        dev = DeviceGraph(solver="pcg", pcg_tol=1e-10, cond=args.cond)
    dev.set_poses(init)
    build = []
    for _ in range(args.builds):
        t0 = time.perf_counter()
        if odom is None:
            dev.set_edges(edges)                   # the call a parent library has
        else:
            dev.set_edges(edges, odometry=odom)
        build.append((time.perf_counter() - t0) * 1e3)
    dev.update()                                   # warm-up (cold cond estimate, allocations)
    upd, lin, asm, sol, its, calc = [], [], [], [], [], True
    for _ in range(args.updates):
        dev.set_poses(init)
        t0 = time.perf_counter()
        st = dev.update()
        upd.append((time.perf_counter() - t0) * 1e3)
        t = dev.timing()
        lin.append(t["linearize_ms"])
        asm.append(t["assemble_ms"])
        sol.append(t["solve_ms"])
        its.append(t["pcg_iterations"])
        calc = calc and st[0]
    out = dict(odom=int(args.odom), is_calc=bool(calc), build_ms=float(np.median(build[1:] or build)),
               build_first_ms=float(build[0]), update_ms=float(np.median(upd)),
               update_min_ms=float(np.min(upd)), linearize_ms=float(np.median(lin)),
               assemble_ms=float(np.median(asm)), solve_ms=float(np.median(sol)),
               pcg_iterations=int(np.median(its)), cond=float(st[3]), edges=int(dev.n_edges),
               n_times=int(len(dev.get_system(dense=False)[0])))
    if hasattr(dev._lib, "slam_graph_chi2"):
        dev.set_poses(init)
        dev.chi2()
        c = []
        for _ in range(20):
            t0 = time.perf_counter()
            tot = dev.chi2()
            c.append((time.perf_counter() - t0) * 1e3)
        out.update(chi2_call_ms=float(np.median(c)), chi2=tot["chi2"])
    dev.close()
    print(json.dumps(out))


def run_child(graph, odom, args, lib=None, cond="estimate"):
    env = dict(os.environ)
    if lib:
        env["SLAM_HIP_LIB"] = os.path.abspath(lib)
    else:
        env.pop("SLAM_HIP_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--graph", graph, "--odom", str(int(odom)),
           "--updates", str(args.updates), "--builds", str(args.builds), "--cond", cond]
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
    ap.add_argument("--updates", type=int, default=7)
    ap.add_argument("--builds", type=int, default=4)
    ap.add_argument("--cond", default="estimate")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_odom_ab.txt"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    from slamhip.graph import circle_graph, circle_graph_odometry
    init, truth, edges = circle_graph(50000, n_landmarks=64, seed=0, odom_noise=0.002)
    odom = circle_graph_odometry(truth, SIGMA, 0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    with tempfile.TemporaryDirectory() as tmp:
        graph = os.path.join(tmp, "c5.npz")
        np.savez(graph, init=init, edges=edges, odom=odom)
        say("graph: 50000 poses, %d pair edges, %d odometry edges (sigma %g %g %g), PCG path (pcg_tol "
            "1e-10), cond=\"estimate\"; %d updates per process after one warm-up, every one from the "
            "initial poses, medians; the structure build is the median of set_edges calls 2..%d; chi2 at "
            "the initial poses" % (len(edges), len(odom), *SIGMA, args.updates, args.builds))
        say()
        say("edge set         E   times   build ms (wall)   first build ms   linearise ms   assemble ms   "
            "solve ms   update ms (wall)   PCG it   cond estimate   chi2 call ms (wall)   sum chi2")
        rows = {}
        for od in (0, 1):
            r = rows[od] = run_child(graph, od, args)
            say("%-10s %7d %7d %17.3f %16.3f %14.4f %13.4f %10.3f %18.3f %8d %15.4g %21.4f %12.5e%s" % (
                "pairs+odom" if od else "pairs", r["edges"], r["n_times"], r["build_ms"],
                r["build_first_ms"], r["linearize_ms"], r["assemble_ms"], r["solve_ms"], r["update_ms"],
                r["pcg_iterations"], r["cond"], r["chi2_call_ms"], r["chi2"],
                "" if r["is_calc"] else "   (is_calc = 0)"))
        alone = run_child(graph, 2, args)
        say("linearise launches, each alone between the handle's events: landmark (%d columns) %.4f ms, "
            "odometry (%d columns, no pair edge in the set) %.4f ms; both in one set %.4f ms" % (
                rows[0]["edges"], rows[0]["linearize_ms"], alone["edges"], alone["linearize_ms"],
                rows[1]["linearize_ms"]))
        a, b = rows[0], rows[1]
        say("with odometry against without: build %+.1f %%, linearise %+.4f ms, "
            "assemble %+.1f %%, update %+.1f %%, PCG iterations %d -> %d, chi2 call %+.1f %%" % (
                100 * (b["build_ms"] / a["build_ms"] - 1), b["linearize_ms"] - a["linearize_ms"],
                100 * (b["assemble_ms"] / a["assemble_ms"] - 1), 100 * (b["update_ms"] / a["update_ms"] - 1),
                a["pcg_iterations"], b["pcg_iterations"], 100 * (b["chi2_call_ms"] / a["chi2_call_ms"] - 1)))
        if args.parent_lib:
            say()
            say("default path (no odometry edges, cond=\"margin\") against the parent commit's library, "
                "interleaved rounds (a fresh process each):")
            say("round   parent update ms   parent linearise ms   parent build ms   this update ms   "
                "this linearise ms   this build ms")
            par, new = [], []
            for i in range(args.rounds):
                p = run_child(graph, 0, args, lib=args.parent_lib, cond="margin")
                n = run_child(graph, 0, args, cond="margin")
                par.append(p)
                new.append(n)
                say("%5d %18.3f %21.4f %17.3f %16.3f %19.4f %15.3f" % (
                    i, p["update_ms"], p["linearize_ms"], p["build_ms"], n["update_ms"], n["linearize_ms"],
                    n["build_ms"]))
            pu = [p["update_ms"] for p in par]
            nu = [n["update_ms"] for n in new]
            med = float(np.median(nu))
            say("parent update ms: min %.3f median %.3f max %.3f; this: min %.3f median %.3f max %.3f" % (
                min(pu), float(np.median(pu)), max(pu), min(nu), med, max(nu)))
            inside = min(pu) <= med <= max(pu)
            say("this median %s the parent's spread [%.3f, %.3f]" % (
                "lies inside" if inside else ("lies BELOW" if med < min(pu) else "lies ABOVE"),
                min(pu), max(pu)))
            pl = [p["linearize_ms"] for p in par]
            nl = [n["linearize_ms"] for n in new]
            say("linearise kernel ms: parent min %.4f median %.4f max %.4f; this min %.4f median %.4f "
                "max %.4f" % (min(pl), float(np.median(pl)), max(pl), min(nl), float(np.median(nl)),
                              max(nl)))
            assert all(p["pcg_iterations"] == n["pcg_iterations"] for p, n in zip(par, new))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
