#!/usr/bin/env python3
"""Timing of the fixed-size path: one 1 GiB device stream at chunk size 4096,
synchronous cdc_chunk_batch_device calls (GiB/s, ms per call).  Diagnostics only."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import chunkfs_amd as c  # noqa: E402

n = 1 << 30
b = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
ch = c.FSChunker(4096)
cap = ch.batch_max_chunks([n])
out = torch.empty((cap, 2), dtype=torch.int64, device="cuda:0")
args = ([b.data_ptr()], [n], out.data_ptr(), cap)
first = ch.chunk_batch_device(*args)
torch.cuda.synchronize()
ts = time.perf_counter()
while time.perf_counter() - ts < 0.08:
    ch.chunk_batch_device(*args)
reps = 50
t0 = time.perf_counter()
for _ in range(reps):
    first = ch.chunk_batch_device(*args)
el = (time.perf_counter() - t0) / reps
t = ch.last_timing()
print(f"fixed  {n / el / 2**30:10.1f} GiB/s  {el * 1e3:.4f} ms/call  kernel {t['total_ms']:.4f} ms  chunks {int(first[1])}",
      flush=True)
ch.close()
