"""Call overhead of the multi-device index: 1000 one-query, k = 10 searches on three logical shards of a 20 000-row
index through both entries, wall microseconds per call -- vaqhip_multi_search (host_entry_us), vaqhip_multi_search_device
(issuing alone: device_entry_issue_us; with the final synchronise: device_entry_us).  Prints one JSON line.
VAQHIP_LIB=<path> measures another build of the library (profiles/multi_split_timing.json).

    python tools/bench_multi_calls.py
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from helpers import make_case  # noqa: E402
from vaq_amd.index import VaqHipMulti  # noqa: E402

c = make_case(601, 64, [8] * 8, 20000, 1)
m = VaqHipMulti([0, 0, 0], c["bits"], c["cents"], c["eig"])
m.set_codes(c["codes"])
q = torch.from_numpy(c["X"]).cuda()
out = (torch.empty((1, 10), dtype=torch.int32, device="cuda"), torch.empty((1, 10), dtype=torch.float32, device="cuda"))
res = {}
for _ in range(50):
    m.search(c["X"], 10)
t0 = time.perf_counter()
for _ in range(1000):
    m.search(c["X"], 10)
res["host_entry_us"] = round((time.perf_counter() - t0) * 1e3, 2)
for _ in range(50):
    m.search_device(q, 10, out=out)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(1000):
    m.search_device(q, 10, out=out)
t1 = time.perf_counter()
torch.cuda.synchronize()
res["device_entry_issue_us"] = round((t1 - t0) * 1e3, 2)
res["device_entry_us"] = round((time.perf_counter() - t0) * 1e3, 2)
print(json.dumps(res), flush=True)
m.close()
