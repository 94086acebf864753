"""Cost of the robust edge weights at the config-5 shape:
circle_graph(50000, n_landmarks=64, seed=0, odom_noise=0.002), PCG path.

  python tools/graph_robust_probe.py [--parent-lib PATH] [--rounds 5] [--out FILE]

Per kind (none, huber 1, cauchy 2, dcs 5), one child process each: the
linearise kernel's device time, the time of a slam_graph_chi2 call (both
launches, the 32-byte read-back and the synchronisation; wall clock) and the
time per Gauss-Newton iteration (slam_graph_update, wall clock), each over
`--updates` updates after one warm-up, the poses reset before every update so
that every update solves the same system.

With --parent-lib (a libslam_hip.so built from the parent commit, loaded
through SLAM_HIP_LIB) the default path is measured against it in interleaved
rounds, one fresh process per library and round; the default path's median
must lie inside the spread (min .. max) of the parent's own rounds.
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

KINDS = [("none", None), ("huber", 1.0), ("cauchy", 2.0), ("dcs", 5.0)]


def child(args):
    from slamhip.graph import DeviceGraph
    g = np.load(args.graph)
    init, edges = g["init"], g["edges"]
    kw = {} if args.kind == "none" else dict(robust=(args.kind, args.param))
    dev = DeviceGraph(solver="pcg", pcg_tol=1e-10, cond=args.cond, **kw)
    dev.set_poses(init)
    dev.set_edges(edges)
    dev.update()                                   # warm-up (cold cond estimate, allocations)
    upd, lin, asm, its, calc = [], [], [], [], True
    for _ in range(args.updates):
        dev.set_poses(init)
        t0 = time.perf_counter()
        st = dev.update()
        upd.append((time.perf_counter() - t0) * 1e3)
        t = dev.timing()
        lin.append(t["linearize_ms"])
        asm.append(t["assemble_ms"])
        its.append(t["pcg_iterations"])
        calc = calc and st[0]
    out = dict(kind=args.kind, is_calc=bool(calc), update_ms=float(np.median(upd)),
               update_min_ms=float(np.min(upd)),
               linearize_ms=float(np.median(lin)), assemble_ms=float(np.median(asm)),
               pcg_iterations=int(np.median(its)), edges=int(len(edges)))
    if not calc:                                   # why the last update was not applied
        g, c = dev.gate_info(), dev.cond_info()
        out["why"] = ("gate: det %s (log det in [%.6g, %.6g]), cond %s (cond %.4g); estimate status "
                      "%d after %d iterations; stats %r" % (g["det"], g["logdet_lo"], g["logdet_hi"],
                                                           g["cond_decided"], g["cond"], c["status"],
                                                           c["iterations"], tuple(st)))
    if hasattr(dev._lib, "slam_graph_chi2"):       # a parent library predates the call
        dev.set_poses(init)                        # every row evaluates the same poses
        dev.chi2()
        c = []
        for _ in range(20):
            t0 = time.perf_counter()
            tot = dev.chi2()
            c.append((time.perf_counter() - t0) * 1e3)
        out.update(chi2_call_ms=float(np.median(c)), chi2=tot["chi2"], cost=tot["cost"],
                   n_low_weight=tot["n_low_weight"])
    dev.close()
    print(json.dumps(out))


def run_child(graph, kind, param, updates, lib=None, cond="margin"):
    env = dict(os.environ)
    if lib:
        env["SLAM_HIP_LIB"] = os.path.abspath(lib)
    else:
        env.pop("SLAM_HIP_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--graph", graph, "--kind", kind,
           "--param", str(param or 0.0), "--updates", str(updates), "--cond", cond]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit("child failed (%d): nothing more is started" % r.returncode)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--graph")
    ap.add_argument("--kind", default="none")
    ap.add_argument("--param", type=float, default=0.0)
    ap.add_argument("--updates", type=int, default=7)
    ap.add_argument("--cond", default="margin")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_robust_ab.txt"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    from slamhip.graph import circle_graph
    init, _, edges = circle_graph(50000, n_landmarks=64, seed=0, odom_noise=0.002)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    with tempfile.TemporaryDirectory() as tmp:
        graph = os.path.join(tmp, "c5.npz")
        np.savez(graph, init=init, edges=edges)
        say("graph: 50000 poses, %d edges, PCG path (pcg_tol 1e-10); %d updates per process after one "
            "warm-up, every one from the initial poses, medians; chi2 at the initial poses"
            % (len(edges), args.updates))
        for cond in ("margin", "estimate"):
            say()
            say("gate: %s" % cond)
            say("kind         linearise ms   assemble ms   update ms (wall)   PCG it   chi2 call ms (wall)"
                "   sum chi2      sum rho       w < 0.1")
            rows = {}
            for kind, param in KINDS:
                r = rows[kind] = run_child(graph, kind, param, args.updates, cond=cond)
                say("%-6s %-4s %12.4f %13.4f %18.3f %8d %21.4f %12.5e %12.5e %9d%s" % (
                    kind, "" if param is None else "%g" % param, r["linearize_ms"], r["assemble_ms"],
                    r["update_ms"], r["pcg_iterations"], r["chi2_call_ms"], r["chi2"], r["cost"],
                    r["n_low_weight"], "" if r["is_calc"] else "   (is_calc = 0)"))
            for kind, _ in KINDS:
                if "why" in rows[kind]:
                    say("%s, is_calc = 0: %s" % (kind, rows[kind]["why"]))
            base = rows["none"]["linearize_ms"]
            say("linearise against none: " + ", ".join(
                "%s %+.1f %%" % (k, 100.0 * (rows[k]["linearize_ms"] / base - 1.0)) for k, _ in KINDS[1:]))
        say()
        say("(the update time of a robust kind is not comparable with none's: the weighted H is another "
            "system, with another PCG iteration count and another estimate)")
        if args.parent_lib:
            say()
            say("default path against the parent commit's library, interleaved rounds (a fresh process "
                "each):")
            say("round   parent update ms   parent linearise ms   this update ms   this linearise ms")
            par, new = [], []
            for i in range(args.rounds):
                p = run_child(graph, "none", None, args.updates, lib=args.parent_lib)
                n = run_child(graph, "none", None, args.updates)
                par.append(p)
                new.append(n)
                say("%5d %18.3f %21.4f %16.3f %19.4f" % (i, p["update_ms"], p["linearize_ms"],
                                                         n["update_ms"], n["linearize_ms"]))
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
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
