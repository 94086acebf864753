"""Cost of the landmark map at the config-5 shape:
circle_graph_halves(50000, n_landmarks=64, seed=0, odom_noise=0.002), every
visible landmark a half-edge.

  python tools/graph_map_probe.py [--parent-lib PATH] [--rounds 5] [--out FILE]

One child process: set_observations (wall clock), then `--evals` landmarks()
evaluations with every output after one warm-up -- the call (wall clock), the
kernels between the handle's events, each and whole -- and the time of a
device-to-device copy that moves as many bytes as the five kernels read and
write (half of them read, half written: a copy of half that size, timed
between events around 20 copies).  The NumPy restatement
(tests/graph_map_ref.py) runs once on the same workload in this process, and
the two maps are compared.  Nothing here is a prediction: the file records
what was found.

With --parent-lib (a libslam_hip.so built from the parent commit, loaded
through SLAM_HIP_LIB) the default path -- circle_graph's pair edges at the same
size, no observations, the default gate -- is measured against it in interleaved
rounds, one fresh process per library and round; this change's median update
time must lie inside the spread (min .. max) of the parent's own rounds.
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
for p in ("slam-robot_simu_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

N_LANDMARKS = 64


def map_bytes(n_grouped, n_chunks, n_landmarks):
    """Bytes the five kernels read and write in one evaluation with every output."""
    g, c, nl = n_grouped, n_chunks, n_landmarks
    contrib = g * (8 + 16 + 24) + g * 40           # pose index, (d, dir), the pose; L and W
    fold = g * 40 + c * 16 + c * 40                # the terms, the chunk table; the chunk sums
    finish = c * 40 + nl * 16 + nl * (16 + 32)     # the chunk sums, the CSRs; mean and cov
    chi2_fold = g * (40 + 8) + c * 16 + g * 8 + c * 8
    chi2_finish = c * 8 + nl * 8 + nl * 8
    return contrib + fold + finish + chi2_fold + chi2_finish


def child_map(args):
    import torch
    torch.cuda.init()                                  # PyTorch's HIP runtime first, as the tests do
    from slamhip.graph import DeviceGraph
    g = np.load(args.graph)
    init, halves = g["init"], g["halves"]
    dev = DeviceGraph(solver="pcg")
    dev.set_poses(init)
    t0 = time.perf_counter()
    dev.set_observations(halves, N_LANDMARKS)
    set_ms = (time.perf_counter() - t0) * 1e3
    out = dev.landmarks(per_observation=True)          # warm-up
    call, ker = [], []
    for _ in range(args.evals):
        t0 = time.perf_counter()
        dev.landmarks(per_observation=True)
        call.append((time.perf_counter() - t0) * 1e3)
        ker.append(dev.map_timing())
    count = out[2]
    chunks = int(np.sum((count + 255) // 256))
    nbytes = map_bytes(int(count.sum()), chunks, N_LANDMARKS)
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    dst.copy_(src)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        dst.copy_(src)
    e1.record()
    torch.cuda.synchronize()
    keys = ("ms", "contrib_ms", "fold_ms", "finish_ms", "chi2_fold_ms", "chi2_finish_ms")
    res = dict(set_ms=set_ms, call_ms=float(np.median(call)), launches=ker[-1]["launches"],
               grouped=int(count.sum()), chunks=chunks, count_min=int(count.min()), count_max=int(count.max()),
               bytes=int(nbytes), copy_ms=e0.elapsed_time(e1) / 20)
    res.update({k: float(np.median([t[k] for t in ker])) for k in keys})
    np.savez(args.result, mean=out[0], cov=out[1], count=out[2], chi2=out[3], half=out[4])
    dev.close()
    print(json.dumps(res))


def child_update(args):
    from slamhip.graph import DeviceGraph
    g = np.load(args.graph)
    init, edges = g["init"], g["edges"]
    dev = DeviceGraph(solver="pcg", pcg_tol=1e-10, cond="margin")
    dev.set_poses(init)
    dev.set_edges(edges)
    dev.update()                                   # warm-up (cold cond estimate, allocations)
    upd, lin, its = [], [], []
    for _ in range(args.updates):
        dev.set_poses(init)
        t0 = time.perf_counter()
        st = dev.update()
        upd.append((time.perf_counter() - t0) * 1e3)
        t = dev.timing()
        lin.append(t["linearize_ms"])
        its.append(t["pcg_iterations"])
    poses = dev.get_poses()
    dev.close()
    print(json.dumps(dict(update_ms=float(np.median(upd)), linearize_ms=float(np.median(lin)),
                          pcg_iterations=int(np.median(its)), is_calc=bool(st[0]),
                          pose_sum=float(np.sum(poses)))))


def run_child(kind, graph, args, lib=None, result=None):
    env = dict(os.environ)
    if lib:
        env["SLAM_HIP_LIB"] = os.path.abspath(lib)
    else:
        env.pop("SLAM_HIP_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--graph", graph,
           "--updates", str(args.updates), "--evals", str(args.evals)]
    if result:
        cmd += ["--result", result]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit("child failed (%d): nothing more is started" % r.returncode)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["map", "update"])
    ap.add_argument("--graph")
    ap.add_argument("--result")
    ap.add_argument("--updates", type=int, default=7)
    ap.add_argument("--evals", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_map_ab.txt"))
    args = ap.parse_args()
    if args.child == "map":
        return child_map(args)
    if args.child == "update":
        return child_update(args)
    from slamhip.graph import circle_graph, circle_graph_halves
    init, truth, halves, _ = circle_graph_halves(50000, n_landmarks=N_LANDMARKS, seed=0, odom_noise=0.002)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    with tempfile.TemporaryDirectory() as tmp:
        graph, result = os.path.join(tmp, "c5.npz"), os.path.join(tmp, "map.npz")
        np.savez(graph, init=init, halves=halves,
                 edges=circle_graph(50000, n_landmarks=N_LANDMARKS, seed=0, odom_noise=0.002)[2])
        r = run_child("map", graph, args, result=result)
        say("world: 50000 poses, %d landmarks, %d half-edges (every visible landmark; %d .. %d per "
            "landmark, %d chunks of 256); the map at the initial poses, every output; %d evaluations "
            "after one warm-up, medians" % (N_LANDMARKS, len(halves), r["count_min"], r["count_max"],
                                            r["chunks"], args.evals))
        say("set_observations (grouping on the host, upload): %.3f ms wall" % r["set_ms"])
        say("landmarks(): %.4f ms wall per call; %d kernels, %.4f ms between the handle's events:" % (
            r["call_ms"], r["launches"], r["ms"]))
        for k, name in (("contrib_ms", "contributions"), ("fold_ms", "fold of the five sums"),
                        ("finish_ms", "mean and cov"), ("chi2_fold_ms", "chi-square and its fold"),
                        ("chi2_finish_ms", "chi-square per landmark")):
            say("  %-26s %.4f ms" % (name, r[k]))
        say("bytes the kernels read and write: %d (%.1f per half-edge); a device-to-device copy moving as "
            "many (half read, half written): %.4f ms; kernels / copy = %.2f" % (
                r["bytes"], r["bytes"] / len(halves), r["copy_ms"], r["ms"] / r["copy_ms"]))
        import graph_map_ref as mr
        rows = np.column_stack([halves["time"], halves["pose"], halves["landmark"], halves["obs"]])
        t0 = time.perf_counter()
        ref = mr.landmark_map(rows.astype(np.float64), N_LANDMARKS, init)
        ref_ms = (time.perf_counter() - t0) * 1e3
        got = np.load(result)
        say("NumPy restatement on this workload: %.0f ms; restatement / landmarks() call = %.0f, / kernels = "
            "%.0f" % (ref_ms, ref_ms / r["call_ms"], ref_ms / r["ms"]))
        say("device against the restatement here: mean %.3g m, cov %.3g of its largest entry, chi2_l %.3g "
            "relative, chi2_k %.3g of max(1, chi2_k)" % (
                np.abs(got["mean"] - ref[0]).max(),
                (np.abs(got["cov"] - ref[1]).reshape(N_LANDMARKS, 4).max(1)
                 / np.abs(ref[1]).reshape(N_LANDMARKS, 4).max(1)).max(),
                (np.abs(got["chi2"] - ref[3]) / ref[3]).max(),
                (np.abs(got["half"] - ref[4]) / np.maximum(1.0, ref[4])).max()))
        if args.parent_lib:
            say()
            say("default path (pair edges of circle_graph at the same size, no observations, "
                "cond=\"margin\", %d updates per process after one warm-up, each from the initial poses, "
                "medians) against the parent commit's library, interleaved rounds (a fresh process each):"
                % args.updates)
            say("round   parent update ms   parent linearise ms   this update ms   this linearise ms")
            par, new = [], []
            for i in range(args.rounds):
                p = run_child("update", graph, args, lib=args.parent_lib)
                n = run_child("update", graph, args)
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
            same = all(p["pcg_iterations"] == n["pcg_iterations"] and p["pose_sum"] == n["pose_sum"]
                       for p, n in zip(par, new))
            say("PCG iterations and the sum of the updated poses: %s in every round" % (
                "identical" if same else "DIFFERENT"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
