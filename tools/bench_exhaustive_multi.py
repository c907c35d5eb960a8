"""The exhaustive form across the shards of a multi-device refiner (vaqhip_multi_refiner_search_device) next to the
single refiner's (vaqhip_refiner_search_device) on the same rows.

    python tools/bench_exhaustive_multi.py --out profiles/exhaustive_multi_1m.json

Workload: 1M x 128 sift_like rows, k = 100, 100 and 10 000 queries without exact_ties; a tie-heavy run (rows drawn from
1000 integer vectors) of 100 queries with exact_ties, where the chain of replays runs.  G = 1, 2, 4, 8 shards over
distinct GPUs where the machine has that many, LOGICAL shards on GPU 0 otherwise -- every run says which.  With logical
shards the figures are the cost of the mechanism (more launches, the gather, the cross-shard merge, the hand-over), not
scaling: the shards share one GPU.  Device events, median of the repetitions after warm-up, the single and the multi
form alternating in one process; the single form measured in the same run is the yardstick.  The two answers are
compared for equality first.  The phases are the refiner's own events (option "timing", one more call afterwards).
Nothing is fixed in advance: the file holds what was measured."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--queries", default="100,10000")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--shards", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--exact-queries", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exhaustive_multi_1m.json"))
    a = ap.parse_args()

    import torch
    import vaq_amd
    from vaq_amd import build, harness
    if not torch.cuda.is_available():
        print("bench_exhaustive_multi: no GPU: nothing is measured", file=sys.stderr)
        return 1
    N, D, k = a.rows, a.dim, a.k
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    n_gpus = torch.cuda.device_count()
    nqs = [int(x) for x in a.queries.split(",")]
    out = {"tool": "tools/bench_exhaustive_multi.py", "rows": N, "dim": D, "k": k, "reps": a.reps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "gpus": n_gpus, "source_hash": build.source_hash(),
           "timing": "device events, median of %d after %d warm-up calls, single and multi alternating in one process"
                     % (a.reps, a.warmup),
           "note": "logical shards share one GPU: their figures are the cost of the mechanism, not scaling", "runs": []}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for data in ("sift_like", "tie_heavy"):
        if data == "sift_like":
            rows = harness.sift_like(N, D, stream=0, device=dev)
            queries = harness.sift_like(max(nqs), D, stream=1, device=dev)
            legs = [(n, 0) for n in nqs]
        else:
            g = torch.Generator(device=dev)
            g.manual_seed(17)
            base = torch.randint(0, 256, (1000, D), generator=g, device=dev).float()
            rows = base[torch.randint(0, 1000, (N,), generator=g, device=dev)].contiguous()
            queries = torch.randint(0, 256, (max(nqs), D), generator=g, device=dev).float()
            legs = [(min(a.exact_queries, max(nqs)), 1)] if a.exact_queries > 0 else []
        one = vaq_amd.VaqRefiner(D)
        one.set_rows(rows)
        rows_h = rows.cpu().numpy()
        del rows
        for G in a.shards:
            distinct = n_gpus >= G
            m = vaq_amd.VaqMultiRefiner(list(range(G)) if distinct else [0] * G, D)
            m.set_rows(rows_h)
            for nq, exact in legs:
                q = queries[:nq].contiguous()
                one.exact_ties = m.exact_ties = bool(exact)
                o1 = (torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), device=dev))
                om = (torch.empty_like(o1[0]), torch.empty_like(o1[1]))
                calls = {"single": lambda: one.search_device(q, k, out=o1), "multi": lambda: m.search_device(q, k, out=om)}
                for fn in calls.values():
                    fn()
                torch.cuda.synchronize()
                assert torch.equal(o1[0], om[0]) and torch.equal(o1[1].view(torch.int32), om[1].view(torch.int32)), \
                    "the sharded answer differs from the single form's"
                times = {n: [] for n in calls}
                for it in range(a.warmup + a.reps):
                    for n, fn in calls.items():  # alternated: one of each per repetition
                        ms = timed(fn)
                        if it >= a.warmup:
                            times[n].append(ms)
                phases = {}
                for n, r in (("single", one), ("multi", m)):
                    r.set_option("timing", 1)
                    calls[n]()
                    phases[n] = {f: (round(v, 4) if isinstance(v, float) else v) for f, v in r.last_search_timing().items()}
                    r.set_option("timing", 0)
                run = {"data": data, "queries": nq, "exact_ties": exact, "shards": G,
                       "placement": "distinct GPUs" if distinct else "logical shards on GPU 0", "equal_to_single": True,
                       "single_ms": stats(times["single"]), "multi_ms": stats(times["multi"]),
                       "single_spread_ms": round(max(times["single"]) - min(times["single"]), 4),
                       "multi_minus_single_ms": round(statistics.median(times["multi"]) - statistics.median(times["single"]), 4),
                       "single_phases": phases["single"], "multi_phases": phases["multi"],
                       "gathered_bytes": (G - 1) * nq * (k + exact) * 8,
                       "state_bytes_per_hop": nq * k * 8 if exact and G > 1 else 0}
                out["runs"].append(run)
                print(json.dumps(run), flush=True)
            m.close()
        one.close()
        del rows_h, queries
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
