"""What reconstructing the ancestral states of every inner node costs (profiles/ancestral.json): the calling pattern of
RAxML-NG --ancestral / pll-modules - for each inner node a short partial traversal that turns the CLVs towards it, then
that node's sites x states table - on 64 taxa x 100k sites DNA (BASELINE configs[1]'s shape) and 64 taxa x 50k sites,
20 states (configs[2]'s shape), random topologies.

Per shape, on the GPU (one child process under its own `timeout`):
  * us per node of the loop over all inner nodes, partial traversal included: pll_gpu_node_ancestral_async into slices
    of one device buffer with ONE synchronisation at the end; pll_compute_node_ancestral (table copied back per node);
    and - the yardstick - the same partial traversals followed by one pll_compute_edge_loglikelihood each, which is what
    the library could do for such a caller before these entry points existed;
  * us per call with the traversal excluded (the same edge again and again, CLVs in place);
  * kernel launches per node, the kernel's time by HIP events, its algorithmic bytes and their share of 8 TB/s;
  * a plain device-to-host copy of one table, for the difference between the synchronous and the stream-ordered call.
On the host (another child process): the reference's AVX2 pll_compute_node_ancestral for the same calls, one core.

Usage: python tools/ancestral_timing.py [--out profiles/ancestral.json] [--rounds 5]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "libpll-2_amd"), ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
from pllamd import api, workload as W  # noqa: E402
from test_gpu_tree_search import Driven  # noqa: E402
from utree import UTree  # noqa: E402

PEAK_BYTES_PER_S = 8e12
SHAPES = {
    "dna_64x100k": dict(states=4, tips=64, sites=100000, note="64 taxa x 100k sites, 4 states x 4 rates (BASELINE configs[1]'s shape)"),
    "aa_64x50k": dict(states=20, tips=64, sites=50000, note="64 taxa x 50k sites, 20 states x 4 rates (BASELINE configs[2]'s shape)"),
}


def build(lib, shape, seed=11):
    rng = np.random.Generator(np.random.PCG64(seed))
    tree = UTree(shape["tips"], rng)
    states = shape["states"]
    st = W.random_states(shape["tips"], shape["sites"], states, seed + 1, 15)
    if states == 4:
        seqs, cmap, exch, freqs = W.states_to_sequences(st, W.NT_CHARS), W.map_nt(), W.GTR_DNA["exch"], W.GTR_DNA["freqs"]
    else:
        exch, freqs = W.synthetic_exch(states)
        seqs, cmap = W.states_to_sequences(st, W.AA_CHARS), W.map_aa()
    d = Driven(lib, tree, states, shape["sites"], 0, seqs, cmap, exch, freqs, W.gamma_rates_mean(0.5, 4))
    return tree, d


def passes(tree, count):
    """`count` passes over all inner nodes: per node (operations of its partial traversal, edge arguments). From the
    third pass on every pass starts from the state the one before left, so all of them are the same lists."""
    out = []
    for _ in range(count):
        out.append([(tree.ops_for(rec), tree.edge_args(rec)) for rec in tree.inner_nodes])
    return out


def gpu_step(name, rounds):
    shape = SHAPES[name]
    lib = api.PllLib()
    hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
    tree, d = build(lib, shape)
    sites, states = shape["sites"], shape["states"]
    table = sites * states * 8
    plan = passes(tree, 2 + 4 * rounds)
    nodes = len(plan[0])
    dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), C.c_size_t(nodes * table)) == 0
    host = np.zeros((sites, states))
    fi = api.uptr(d.params)
    ops_arrays = [[(api.make_ops(ops), len(ops), edge) for ops, edge in p] for p in plan]
    us = lambda t0, n: (time.perf_counter() - t0) * 1e6 / n

    def traversal(arr, n):
        if n:
            lib.pll_update_partials(d.p, arr, n)

    def run_async(p):
        t0 = time.perf_counter()
        for i, (arr, n, e) in enumerate(p):
            traversal(arr, n)
            assert lib.pll_gpu_node_ancestral_async(d.p, e[0], e[1], e[2], e[3], e[4], fi, C.c_void_p(dev.value + i * table))
        assert lib.pll_gpu_synchronize(d.p)
        return us(t0, len(p))

    def run_sync(p):
        t0 = time.perf_counter()
        for arr, n, e in p:
            traversal(arr, n)
            assert lib.pll_compute_node_ancestral(d.p, e[0], e[1], e[2], e[3], e[4], fi, api.dptr(host))
        return us(t0, len(p))

    def run_lnl(p):
        t0 = time.perf_counter()
        for arr, n, e in p:
            traversal(arr, n)
            lib.pll_compute_edge_loglikelihood(d.p, e[0], e[1], e[2], e[3], e[4], fi, None)
        return us(t0, len(p))

    def run_traversal(p):
        t0 = time.perf_counter()
        for arr, n, e in p:
            traversal(arr, n)
        assert lib.pll_gpu_synchronize(d.p)
        return us(t0, len(p))

    try:
        run_sync(ops_arrays[0])  # the full traversal, every buffer allocated
        run_async(ops_arrays[1])
        res = {"async": [], "sync": [], "edge_lnl": [], "traversal_only": []}
        k = 2
        for _ in range(rounds):  # alternating, same box, same state at the start of every pass
            for key, fn in (("edge_lnl", run_lnl), ("async", run_async), ("sync", run_sync), ("traversal_only", run_traversal)):
                res[key].append(fn(ops_arrays[k]))
                k += 1
        # launches: the traversal's, then one per table
        launches_trav, launches_anc = [], []
        for arr, n, e in ops_arrays[-1]:
            traversal(arr, n)
            before = lib.pll_gpu_last_launch_count(d.p) if n else 0
            launches_trav.append(before)
            lib.pll_gpu_synchronize(d.p)
            b2 = lib.pll_gpu_last_launch_count(d.p)
            assert lib.pll_gpu_node_ancestral_async(d.p, e[0], e[1], e[2], e[3], e[4], fi, dev)
            launches_anc.append(lib.pll_gpu_last_launch_count(d.p) - b2)
        lib.pll_gpu_synchronize(d.p)
        # the calls alone: CLVs in place, the same edge `reps` times
        e = ops_arrays[-1][-1][2]
        reps = 200
        alone = {}
        for _ in range(3):
            t0 = time.perf_counter()
            for _i in range(reps):
                lib.pll_gpu_node_ancestral_async(d.p, e[0], e[1], e[2], e[3], e[4], fi, dev)
            lib.pll_gpu_synchronize(d.p)
            alone.setdefault("async", []).append(us(t0, reps))
            t0 = time.perf_counter()
            for _i in range(reps):
                lib.pll_compute_node_ancestral(d.p, e[0], e[1], e[2], e[3], e[4], fi, api.dptr(host))
            alone.setdefault("sync", []).append(us(t0, reps))
            t0 = time.perf_counter()
            for _i in range(reps):
                lib.pll_compute_edge_loglikelihood(d.p, e[0], e[1], e[2], e[3], e[4], fi, None)
            alone.setdefault("edge_lnl", []).append(us(t0, reps))
            t0 = time.perf_counter()
            for _i in range(reps):
                assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), dev, C.c_size_t(table), 2) == 0
            alone.setdefault("d2h_copy", []).append(us(t0, reps))
        # the kernel by HIP events: `reps` launches between one start and one stop
        kern = []
        for _ in range(3):
            lib.pll_gpu_synchronize(d.p)
            lib.pll_gpu_timer_start(d.p)
            for _i in range(reps):
                lib.pll_gpu_node_ancestral_async(d.p, e[0], e[1], e[2], e[3], e[4], fi, dev)
            kern.append(lib.pll_gpu_timer_stop(d.p) * 1e3 / reps)
        other_is_tip = e[2] < shape["tips"]
        clv = sites * 4 * states * 8
        bytes_alg = clv + (sites if other_is_tip else clv) + table
        kernel_us = min(kern)
        med = lambda v: round(statistics.median(v), 2)
        out = {
            "shape": shape["note"], "inner_nodes": nodes, "table_bytes": table,
            "ops_per_partial_traversal_mean": round(float(np.mean([n for _, n, _ in ops_arrays[-1]])), 2),
            "us_per_node_with_traversal": {k: {"median": med(v), "min": round(min(v), 2), "all": [round(x, 2) for x in v]} for k, v in res.items()},
            "us_per_call_without_traversal": {k: {"median": med(v), "min": round(min(v), 2)} for k, v in alone.items()},
            "launches_per_node": {"partial_traversal_mean": round(float(np.mean(launches_trav)), 2), "ancestral": max(launches_anc)},
            "kernel": {"us_by_events_back_to_back": round(kernel_us, 2), "other_end": "tip codes" if other_is_tip else "CLV",
                       "algorithmic_bytes": bytes_alg, "fraction_of_8TBps": round(bytes_alg / (kernel_us * 1e-6) / PEAK_BYTES_PER_S, 3)},
        }
        out["checks"] = {
            "async_loop_not_slower_than_traversal_plus_edge_lnl": out["us_per_node_with_traversal"]["async"]["median"] <= out["us_per_node_with_traversal"]["edge_lnl"]["median"],
            "sync_minus_async_us": round(out["us_per_call_without_traversal"]["sync"]["median"] - out["us_per_call_without_traversal"]["async"]["median"], 2),
            "d2h_copy_us": out["us_per_call_without_traversal"]["d2h_copy"]["median"],
        }
        print(json.dumps(out))
    finally:
        hip.hipFree(dev)
        d.close()


def ref_step(name, calls=6):
    shape = SHAPES[name]
    path = os.path.join(ROOT, "oracle", "_ref", "libpll_ref.so")
    lib = api.PllLib(path)
    tree, d = build(lib, shape)
    sites, states = shape["sites"], shape["states"]
    host = np.zeros((sites, states))
    fi = api.uptr(d.params)
    try:
        plan = passes(tree, 1)[0]
        ts, tt = [], []
        for ops, e in plan[:calls]:
            t0 = time.perf_counter()
            d.update(ops)
            t1 = time.perf_counter()
            assert lib.pll_compute_node_ancestral(d.p, e[0], e[1], e[2], e[3], e[4], fi, api.dptr(host))
            ts.append((time.perf_counter() - t1) * 1e6)
            tt.append((t1 - t0) * 1e6)
        print(json.dumps({"library": "reference, AVX2, one core", "calls": len(ts), "us_per_call_median": round(statistics.median(ts), 1),
                          "us_per_call_min": round(min(ts), 1), "us_partial_traversal_median_after_the_first": round(statistics.median(tt[1:]), 1)}))
    finally:
        d.close()


def child(args, seconds):
    cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"step {args} ended with status {r.returncode}: nothing more is started")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ancestral.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--gpu-step")
    ap.add_argument("--ref-step")
    ap.add_argument("--no-reference", action="store_true")
    a = ap.parse_args()
    if a.gpu_step:
        return gpu_step(a.gpu_step, a.rounds)
    if a.ref_step:
        return ref_step(a.ref_step)
    result = {"what": "marginal ancestral states of every inner node; tools/ancestral_timing.py", "peak_bytes_per_s": PEAK_BYTES_PER_S, "shapes": {}}
    for name in SHAPES:
        entry = child(["--gpu-step", name, "--rounds", str(a.rounds)], 240)
        if not a.no_reference and os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libpll_ref.so")):
            entry["reference"] = child(["--ref-step", name], 240)
        result["shapes"][name] = entry
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result["shapes"], indent=1))


if __name__ == "__main__":
    main()
