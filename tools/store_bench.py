#!/usr/bin/env python3
"""Chunk-store throughput on one GPU: put and get against the device's own copy.

Workload: one splitmix64 device stream (1 GiB by default), FastCDC
4096/8192/16384, every chunk unique.  Timed warm, with HIP events on one
stream:

  (a) put_batch_device of the whole stream into an empty store
      (precheck + index insert + scans + the copy into the arena);
  (b) get_device of the whole file (lookup + scans + the copy out);
  (c) hipMemcpyAsync device-to-device of the same bytes, in the same process
      -- the yardstick: the device's own copy of the same data;
  (d) cdc_file_write_device of the whole stream into an empty file layer
      (chunking + SHA-256 + put + span append: (d) includes the chunking and
      hashing that (a) is handed ready-made, so the two are not compared);
  (e) cdc_file_read_complete_device of that file (range planner + the copy:
      no digest lookup, no host check before the copy) -- compare with (b);
  (f) cdc_file_read_device looped over the file, reported per 1 MiB segment.

Also timed, to separate the copy kernel from the bookkeeping around it:
contains_device (the lookup alone) and get_device with out_cap = 0 (lookup +
scans, no copy); (b) minus the latter is the copy kernel plus the spans.  The
per-kernel split of put comes from a profiler's kernel trace of
`store_bench.py --iters 2 --warmup 1` (kernel names: copy_kernel,
precheck_kernel, scan_*_kernel, lookup_kernel, claim/verify/mark_kernel).

Scrub stage (skipped with --no-scrub), on file systems of their own with a
target store, the file written again before every timed scrub:

  (g) scrub COPY of the whole store (container list + put into the target from
      the base arena + marking);
  (h) cdc_file_read_complete_device after COPY -- the same piece count and
      bytes as (e), reported as a ratio to (e), with its planner-only time;
  (i) scrub RECHUNK with FastCDC 1024/2048/4096 at three group sizes
      (CHUNKFS_AMD_SCRUB_GROUP), to choose the default group;
  (j) cdc_file_read_complete_device and 4 KiB cdc_file_pread_device calls after
      RECHUNK at the default group (about avg / sub-avg times the pieces).

Bench fixture, on the file of (d)-(f), in the same run:

  (k) cdc_file_verify_device of the whole file against its source buffer
      (range planner + the compare kernel: 2 bytes read, none written per byte);
  (l) the alternative that needs no new kernel: (e) followed by a device
      compare of the two buffers (torch.equal) -- compare (k) with it and with
      (e) and (c);
  (m) cdc_files_get_to_dedup_ratio at ratio 4 (the derived file is replaced by
      every call; its span table is allocated inside the call);
  (n) cdc_store_size_distribution_device at adjustment 1024.

Many files (skipped with --no-batch-write), each leg on a fresh layer and store,
FastCDC 4096/8192/16384, file i filled with splitmix64 seeded i:

  (o) 1024 files x 64 KiB written by a loop of cdc_file_write_device and by
      one cdc_files_write_batch_device;
  (p) 16 files x 64 MiB, written the same two ways.

(o) and (p) are wall time around the calls, with a device synchronisation on
both sides (the loop is host-bound: events on one stream would not see the
host's share); the layer is cleared and the files are created outside the
timed window, and the loop and the batch alternate.  Median of 10 after a
warm-up.

Remove and collect (skipped with --no-collect), on a layer of its own written
afresh before every timed collect:

  (q) files A (the stream above) and B (a second stream of the same size),
      remove A, cdc_files_collect: nearly every surviving byte moves, by as
      much as A was long;
  (r) 1024 files of 1/1024 of the stream each, every second one removed,
      cdc_files_collect: many small gaps.

(q) and (r) report the call's own wall time (every pass and host wait in it),
the bytes moved, the move groups, and the ratio to (c) scaled to the bytes moved.

Editing in place (skipped with --no-splice), on a layer of its own holding the
1 GiB file of (d):

  (s) cdc_file_splice_device overwriting 4 KiB in the middle of the file;
  (t) the same inserting 4 KiB there;
  (u) the same deleting 4 KiB there.

Each reports ms, rounds, window_bytes, spans_removed / spans_inserted and the
split of the last call into planner, chunk, resync, hash + put and table build.
Compare with (d): writing the whole file again is the only other way to make
the same edit.

Snapshots and diffs (skipped with --no-snapshot), on a layer of its own holding
the 1 GiB file of (d):

  (v) cdc_files_clone of the file (the clone is removed before each turn);
  (w) cdc_files_diff_device of a clone against the original after one 4 KiB
      overwrite in the middle, exact and with CDC_DIFF_TABLES_ONLY;
  (x) the same call on two unrelated 1 GiB files: every byte is compared.

Compare (v) with (d), writing the same bytes again under another name, and (w),
(x) with the read_plus_verify legs beside them: read_complete_device of one file
plus cdc_file_verify_device of the other, which names the first differing byte only.

Packs (skipped with --no-pack), on a sending layer holding the 1 GiB file of (d)
and a receiving layer of the same size:

  (y) cdc_file_pack_device of the whole file -- compare with (b), the store's get
      of the same bytes;
  (z) the same against a clone, after the 4 KiB overwrite of (s): the pack of an
      incremental backup;
  (aa) cdc_files_unpack_device of the full pack into an empty store, with
      CDC_UNPACK_TRUST -- compare with (a), the put -- and with the SHA-256 check
      -- compare with (d), the whole write (the store is cleared before each turn);
  (ab) cdc_files_unpack_device of the incremental pack into a store that holds
      the base (the file is removed and the store collected before each turn).

Each reports ms (HIP events around the call on its stream), the call's own wall
time, its stats and cdc_debug_pack_split of the last call: wall time between the
call's host waits.

The two hashers (skipped with --no-hash, alone with --only-hash), SHA-256 and
BLAKE2sp in the same run, each leg on layers of its own per hasher:

  (ac) hash_ms of cdc_hash_batch_device over 4 chunks of 16 KiB, and over one;
  (ad) the 4 KiB overwrite of (s);
  (ae) the incremental unpack with the check of (ab);
  (af) the whole write of (d);
  (ag) hash_ms over config 3's chunk list (RabinCDC 2/4/8 KiB over a 256 MiB base
       and 15 edited copies, about 4 GiB), the two hashers alternating.

Each reports the median and the min-max per hasher and SHA-256's time over
BLAKE2sp's; the two conditions of DESIGN.md "Hashers" are evaluated at the end.

The content-aligned delta (skipped with --no-delta, alone with --only-delta), on a
layer of its own holding the 1 GiB file of (d) and an unrelated one:

  (ah) cdc_files_delta_device of a clone against the original after a 4 KiB
       overwrite in the middle, exact and with CDC_DELTA_TABLES_ONLY;
  (ai) the same after a 4 KiB insert; (aj) the same after a 4 KiB delete;
  (ak) the delta of the two unrelated files;
  (al) the delta of the file against the same bytes cut by FastCDC 2/4/8 KiB:
       hardly a slot in common, every byte compared and equal, one COPY.

Beside each, in the same run, cdc_files_diff_device of the same pair -- after the
insert and the delete it compares the half of the file behind the edit and calls
it changed -- and for (ak) also read_complete_device plus cdc_file_verify_device.

Prints one JSON line; --out also writes it to a file.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _hip_runtime():
    """The HIP runtime already mapped into this process (torch's or the system's)."""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime is loaded")


def _group_env(spec):
    cnt, nbytes = spec.split(",")
    mult = {"k": 1 << 10, "m": 1 << 20}.get(nbytes[-1].lower())
    return f"{int(cnt)},{int(nbytes[:-1]) * mult if mult else int(nbytes)}"


def scrub_legs(a, c, L, P, ch, buf, out, n, k, sp, timed, med, fread_ms):
    """Legs (g)-(j): the same stream in file systems with a target store."""
    import torch

    def file_system(scrubber):
        return c.FileSystem.new_with_scrubber(scrubber, max_chunks=k, arena_bytes=n + 16 * k,
                                              target_max_chunks=n // 1024 + 2 * k,
                                              target_arena_bytes=n + n // 64 + 16 * k)

    state = {}

    def rewrite():
        state["fs"].clear_file_system()
        state["w"] = state["fs"].create_file("bench", ch)
        assert L.cdc_file_write_device(state["w"]._fh, ch._h, P(buf.data_ptr()), n, P(sp)) == k

    def do_scrub():
        assert state["fs"].store.scrub(state["scrubber"], stream=sp).processed_data == n

    def do_read():
        assert L.cdc_file_read_complete_device(state["w"]._fh, P(out.data_ptr()), n, None, P(sp)) == n

    def do_size():
        assert L.cdc_file_read_complete_device(state["w"]._fh, None, 0, None, P(sp)) == n

    def do_preads():
        for i in range(256):
            off = (i * 0x9E3779B1) % (n - 4096)
            assert L.cdc_file_pread_device(state["w"]._fh, off, 4096, P(out.data_ptr()), P(sp)) == 4096

    def check_equal(what):
        out.zero_()
        do_read()
        torch.cuda.synchronize()
        if not torch.equal(out, buf):
            raise SystemExit(f"store_bench: the file read back after {what} differs")

    def scrub_times():
        return timed(do_scrub, before=rewrite, iters=a.scrub_iters, warmup=1)

    gib = n / (1 << 30)
    res = {"scrub_iters": a.scrub_iters}
    state["scrubber"] = c.CopyScrubber()
    state["fs"] = file_system(state["scrubber"])
    t = scrub_times()
    res.update(scrub_copy_ms=med(t), scrub_copy_ms_min_max=[min(t), max(t)], scrub_copy_GiBps=gib / (med(t) * 1e-3))
    check_equal("COPY")
    t, tz = timed(do_read), timed(do_size)
    res.update(copy_read_ms=med(t), copy_read_ms_min_max=[min(t), max(t)], copy_read_size_only_ms=med(tz),
               copy_read_copy_ms=med(t) - med(tz), copy_read_vs_file_read=med(t) / fread_ms)

    state.pop("w")._close()
    state["scrubber"] = c.RechunkScrubber(c.FastChunker(c.SizeParams(1024, 2048, 4096)))
    state["fs"] = file_system(state["scrubber"])  # a second file system; the first one is released here
    old = os.environ.pop("CHUNKFS_AMD_SCRUB_GROUP", None)
    res["scrub_rechunk"] = {}
    try:
        for spec in a.scrub_groups.split(";"):
            os.environ["CHUNKFS_AMD_SCRUB_GROUP"] = _group_env(spec)
            t = scrub_times()
            res["scrub_rechunk"][spec] = {"ms": med(t), "ms_min_max": [min(t), max(t)], "GiBps": gib / (med(t) * 1e-3)}
    finally:
        os.environ.pop("CHUNKFS_AMD_SCRUB_GROUP", None)
        if old is not None:
            os.environ["CHUNKFS_AMD_SCRUB_GROUP"] = old
    t = scrub_times()  # the default group
    x = state["fs"].store.scrub_stats()
    res.update(scrub_rechunk_default_ms=med(t), scrub_rechunk_default_ms_min_max=[min(t), max(t)],
               rechunk_keys=x["keys"], rechunk_target_values=x["target_values"])
    check_equal("RECHUNK")
    t, tz, tp = timed(do_read), timed(do_size), timed(do_preads)
    res.update(rechunk_read_ms=med(t), rechunk_read_ms_min_max=[min(t), max(t)], rechunk_read_size_only_ms=med(tz),
               rechunk_read_vs_file_read=med(t) / fread_ms, rechunk_pread4k_us=med(tp) * 1e3 / 256)
    return res


def batch_write_legs(a, c, L, P, ch):
    """Legs (o)-(p): many files by a loop of single writes and by one batch write."""
    import time

    import numpy as np
    import torch
    from chunkfs_amd import _lib

    res = {}
    for leg, files, size in (("o_1024x64KiB", 1024, 64 << 10), ("p_16x64MiB", 16, 64 << 20)):
        data = torch.empty(files * size, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for i in range(files):
            _lib.check(L.cdc_fill_splitmix64_device(P(data.data_ptr() + i * size), size, i, None))
        cap = ch.batch_max_chunks([size] * files)
        fsys = c.FileSystem(store=c.ChunkStore(cap, files * size + 16 * cap))
        reqs = (_lib.cdc_fwrite_t * files)()
        for i in range(files):
            reqs[i].d_data, reqs[i].len = data.data_ptr() + i * size, size
        counts = (ctypes.c_uint64 * files)()
        state = {}

        def fresh():
            fsys.clear_database()
            state["h"] = [fsys.create_file(f"f{i:04d}", ch) for i in range(files)]
            for i, h in enumerate(state["h"]):
                reqs[i].fh = h._fh.value

        def loop():
            total = 0
            for i, h in enumerate(state["h"]):
                got = L.cdc_file_write_device(h._fh, ch._h, P(data.data_ptr() + i * size), size, None)
                assert got > 0, f"cdc_file_write_device: {got}"
                total += got
            return total

        def batch():
            got = L.cdc_files_write_batch_device(fsys._h, ch._h, files, reqs, counts, None)
            assert got > 0, f"cdc_files_write_batch_device: {got}"
            return got

        def wall(fn):
            fresh()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            spans = fn()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            return ms, spans, fsys.store.stats()["arena_used"]

        t_loop, t_batch = [], []
        for it in range(a.warmup + a.iters):
            (ml, sl, ul), (mb, sb, ub) = wall(loop), wall(batch)
            if (sl, ul) != (sb, ub):
                raise SystemExit(f"store_bench: the batch write and the loop differ ({sl}, {ul}) != ({sb}, {ub})")
            if it >= a.warmup:
                t_loop.append(ml)
                t_batch.append(mb)
        med = lambda v: float(np.median(v))  # noqa: E731
        res[leg] = {"files": files, "file_bytes": size, "spans": sl,
                    "loop_ms": med(t_loop), "loop_ms_min_max": [min(t_loop), max(t_loop)],
                    "batch_ms": med(t_batch), "batch_ms_min_max": [min(t_batch), max(t_batch)],
                    "loop_over_batch": med(t_loop) / med(t_batch),
                    "table_blocks": L.cdc_debug_files_table_blocks(fsys._h)}
        del fsys, data
    return res


def collect_legs(a, c, L, P, ch, buf, n, memcpy_ms):
    """Legs (q)-(r): remove and collect.  Every timed collect runs on a layer
    written afresh; the time is the call's own wall time (cdc_collect_stats_t
    .seconds: every pass, the host waits included), set against the device's own
    copy of as many bytes as the collect moved (leg (c), scaled by the bytes).
    split_ms is cdc_debug_collect_split of the last run: wall time between the
    call's host waits, pass by pass."""
    import time

    import numpy as np
    import torch
    from chunkfs_amd import _lib

    res = {}
    other = torch.empty(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _lib.check(L.cdc_fill_splitmix64_device(P(other.data_ptr()), n, a.seed + 1, None))
    cap = ch.batch_max_chunks([n, n])
    fsys = c.FileSystem(store=c.ChunkStore(cap, 2 * n + 16 * cap))

    def leg(name, fill, remove):
        runs = []
        for it in range(1 + a.collect_iters):
            fsys.clear_database()
            fill()
            for nm in remove():
                fsys.remove_file(nm)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fsys.collect()
            r["call_ms"] = (time.perf_counter() - t0) * 1e3  # with the scratch and the old table freed
            split = (ctypes.c_double * 6)()
            assert L.cdc_debug_collect_split(split, 6) == 6
            r["split_ms"] = dict(zip(("references", "allocation", "sort_plan", "rebuild", "move", "rewrite"), split))
            if it:
                runs.append(r)
        ms = [r["seconds"] * 1e3 for r in runs]
        calls = [r["call_ms"] for r in runs]
        r = runs[-1]
        own = memcpy_ms * r["bytes_moved"] / n  # the device's own copy of the same byte count
        res[name] = {k: r[k] for k in r if k not in ("seconds", "call_ms")}
        res[name].update(collect_ms=float(np.median(ms)), collect_ms_min_max=[min(ms), max(ms)],
                         call_ms=float(np.median(calls)), call_ms_min_max=[min(calls), max(calls)],
                         memcpy_same_bytes_ms=own, collect_over_memcpy=float(np.median(ms)) / own if own else None,
                         moved_GiBps=r["bytes_moved"] / (1 << 30) / (float(np.median(ms)) * 1e-3))

    def two_files():
        for nm, t in (("A", buf), ("B", other)):
            h = fsys.create_file(nm, ch)
            assert L.cdc_file_write_device(h._fh, ch._h, P(t.data_ptr()), n, None) > 0

    files, size = 1024, n // 1024
    reqs = (_lib.cdc_fwrite_t * files)()

    def many_files():
        hs = [fsys.create_file(f"f{i:04d}", ch) for i in range(files)]
        for i, h in enumerate(hs):
            reqs[i].fh, reqs[i].d_data, reqs[i].len = h._fh.value, buf.data_ptr() + i * size, size
        assert L.cdc_files_write_batch_device(fsys._h, ch._h, files, reqs, None, None) > 0

    leg("q_remove_first_of_two", two_files, lambda: ["A"])
    leg("r_remove_every_second_of_1024", many_files, lambda: [f"f{i:04d}" for i in range(0, files, 2)])
    return res


def splice_legs(a, c, L, P, ch, buf, n, k, sp, timed, med):
    """Legs (s)-(u): a 4 KiB overwrite, insert and delete in the middle of the file
    of (d), on a layer of its own.  Every iteration edits the file the one before
    left (an insert grows it by 4 KiB, a delete shrinks it) with 4 KiB it has not
    seen.  ms: HIP events around the call on its stream; wall_ms: the host's
    clock around it; split_ms: cdc_debug_splice_split of the last call."""
    import time

    import numpy as np
    import torch
    from chunkfs_amd import _lib

    edit = 4096
    fresh = torch.empty(edit * 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _lib.check(L.cdc_fill_splitmix64_device(P(fresh.data_ptr()), fresh.numel(), a.seed + 7, None))
    fsys = c.FileSystem(store=c.ChunkStore(k + (1 << 14), n + 16 * k + (256 << 20)))
    w = fsys.create_file("bench", ch)
    assert L.cdc_file_write_device(w._fh, ch._h, P(buf.data_ptr()), n, None) == k
    st = _lib.cdc_splice_stats_t()
    turn = {"i": 0}
    res = {}

    def leg(name, rem, ins):
        wall = []

        def call():
            src = fresh.data_ptr() + (turn["i"] % 64) * edit
            turn["i"] += 1
            t0 = time.perf_counter()
            got = L.cdc_file_splice_device(w._fh, ch._h, n // 2 + 1234, rem, P(src) if ins else None, ins,
                                           ctypes.byref(st), P(sp))
            wall.append((time.perf_counter() - t0) * 1e3)
            assert got >= 0, f"cdc_file_splice_device: {got}"

        ms = timed(call)
        wall = wall[a.warmup:]
        split = (ctypes.c_double * 5)()
        assert L.cdc_debug_splice_split(split, 5) == 5
        res[name] = {"ms": med(ms), "ms_min_max": [min(ms), max(ms)], "wall_ms": float(np.median(wall)),
                     "wall_ms_min_max": [min(wall), max(wall)], "rounds": st.rounds, "window_bytes": st.window_bytes,
                     "spans_removed": st.spans_removed, "spans_inserted": st.spans_inserted,
                     "bytes_new": st.bytes_new, "spans": fsys.stat(w)["spans"],
                     "split_ms": dict(zip(("planner", "chunk", "resync", "hash_put", "table_build"), split))}

    leg("s_overwrite_4k", edit, edit)
    leg("t_insert_4k", 0, edit)
    leg("u_delete_4k", edit, 0)
    return res


def snapshot_legs(a, c, L, P, ch, buf, out, n, k, sp, timed, med):
    """Legs (v)-(x) on a layer of its own holding the file of (d): the clone; the
    diff of a clone against the original after one 4 KiB overwrite, exact and
    from the tables alone; the diff of two unrelated files.  Beside each diff,
    what the same question costs without it: read_complete_device of one file
    plus cdc_file_verify_device of the other (which names the first differing
    byte only), in the same run."""
    import torch
    from chunkfs_amd import _lib

    other = torch.empty(n, dtype=torch.uint8, device="cuda")
    fresh = torch.empty(4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _lib.check(L.cdc_fill_splitmix64_device(P(other.data_ptr()), n, a.seed + 11, None))
    _lib.check(L.cdc_fill_splitmix64_device(P(fresh.data_ptr()), 4096, a.seed + 13, None))
    fsys = c.FileSystem(store=c.ChunkStore(2 * k + (1 << 15), 2 * n + 32 * k + (64 << 20)))
    w = fsys.create_file("bench", ch)
    assert L.cdc_file_write_device(w._fh, ch._h, P(buf.data_ptr()), n, None) == k
    res = {}

    def drop():
        if fsys.file_exists("snap"):
            fsys.remove_file("snap")

    def do_clone():
        got = L.cdc_files_clone(fsys._h, b"bench", b"snap", P(sp))
        assert got == k, f"cdc_files_clone: {got}"

    t = timed(do_clone, before=drop)
    res["v_clone"] = {"ms": med(t), "ms_min_max": [min(t), max(t)], "spans": k, "table_bytes": 52 * k + 8}

    e = fsys.open_file("snap", ch)
    st1 = _lib.cdc_splice_stats_t()
    assert L.cdc_file_splice_device(e._fh, ch._h, n // 2 + 1234, 4096, P(fresh.data_ptr()), 4096, ctypes.byref(st1),
                                    None) >= 0
    o = fsys.create_file("other", ch)
    assert L.cdc_file_write_device(o._fh, ch._h, P(other.data_ptr()), n, None) > 0
    cap = 1024
    d_ranges = torch.empty((cap, 2), dtype=torch.int64, device="cuda")
    st, first = _lib.cdc_diff_stats_t(), ctypes.c_uint64(0)
    torch.cuda.synchronize()

    def diff_leg(name, x, y, flags):
        def call():
            got = L.cdc_files_diff_device(x._fh, y._fh, flags, P(d_ranges.data_ptr()), cap, ctypes.byref(st), P(sp))
            assert got >= 0, f"cdc_files_diff_device: {got}"

        t = timed(call)
        res[name] = dict({f: getattr(st, f) for f, _ in _lib.cdc_diff_stats_t._fields_ if f != "seconds"},
                         ms=med(t), ms_min_max=[min(t), max(t)])

    def base_leg(name, x, y):
        def call():
            assert L.cdc_file_read_complete_device(x._fh, P(out.data_ptr()), n, None, P(sp)) == n
            assert L.cdc_file_verify_device(y._fh, P(out.data_ptr()), n, ctypes.byref(first), P(sp)) == 0

        t = timed(call)
        res[name] = {"ms": med(t), "ms_min_max": [min(t), max(t)], "first_diff": first.value}

    diff_leg("w_diff_after_4k_edit", w, e, 0)
    if res["w_diff_after_4k_edit"]["ranges"] < 1 or res["w_diff_after_4k_edit"]["bytes_differing"] > 4096:
        raise SystemExit("store_bench: the diff after a 4 KiB overwrite does not lie inside the 4 KiB")
    diff_leg("w_diff_after_4k_edit_tables_only", w, e, _lib.CDC_DIFF_TABLES_ONLY)
    base_leg("w_read_plus_verify", w, e)
    diff_leg("x_diff_unrelated", w, o, 0)
    if res["x_diff_unrelated"]["bytes_compared"] != n:
        raise SystemExit("store_bench: two unrelated files share bytes")
    base_leg("x_read_plus_verify", w, o)
    return res


def delta_legs(a, c, L, P, ch, buf, out, n, k, sp, timed, med):
    """Legs (ah)-(ak) on a layer of its own holding the file of (d): the delta of a
    clone against the original after a 4 KiB overwrite, a 4 KiB insert and a 4 KiB
    delete in the middle, exact and from the tables alone, and the delta of two
    unrelated files.  Beside each, the parent's way in the same run: the diff of
    the same pair, and read + verify for the unrelated pair."""
    import torch
    from chunkfs_amd import _lib

    other = torch.empty(n, dtype=torch.uint8, device="cuda")
    fresh = torch.empty(4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _lib.check(L.cdc_fill_splitmix64_device(P(other.data_ptr()), n, a.seed + 11, None))
    _lib.check(L.cdc_fill_splitmix64_device(P(fresh.data_ptr()), 4096, a.seed + 13, None))
    fsys = c.FileSystem(store=c.ChunkStore(5 * k + (1 << 15), 3 * n + 80 * k + (64 << 20)))
    w = fsys.create_file("bench", ch)
    assert L.cdc_file_write_device(w._fh, ch._h, P(buf.data_ptr()), n, None) == k
    o = fsys.create_file("other", ch)
    assert L.cdc_file_write_device(o._fh, ch._h, P(other.data_ptr()), n, None) > 0
    cap = 1024
    d_ops = torch.empty((cap, 3), dtype=torch.int64, device="cuda")
    d_ranges = torch.empty((cap, 2), dtype=torch.int64, device="cuda")
    st, ds, first = _lib.cdc_delta_stats_t(), _lib.cdc_diff_stats_t(), ctypes.c_uint64(0)
    torch.cuda.synchronize()
    res = {}

    def delta_leg(name, x, y, flags):
        def call():
            got = L.cdc_files_delta_device(x._fh, y._fh, flags, P(d_ops.data_ptr()), cap, ctypes.byref(st), P(sp))
            assert 0 <= got <= cap, f"cdc_files_delta_device: {got}"

        t = timed(call)
        res[name] = dict({f: getattr(st, f) for f, _ in _lib.cdc_delta_stats_t._fields_ if f != "seconds"},
                         ms=med(t), ms_min_max=[min(t), max(t)])
        return res[name]

    def diff_leg(name, x, y):
        def call():
            assert L.cdc_files_diff_device(x._fh, y._fh, 0, P(d_ranges.data_ptr()), cap, ctypes.byref(ds), P(sp)) >= 0

        t = timed(call)
        res[name] = {"ms": med(t), "ms_min_max": [min(t), max(t)], "bytes_compared": ds.bytes_compared,
                     "bytes_differing": ds.bytes_differing}

    mid = n // 2 + 1234
    for label, rem, ins in (("ah_overwrite", 4096, 4096), ("ai_insert", 0, 4096), ("aj_delete", 4096, 0)):
        name = "snap_" + label
        assert L.cdc_files_clone(fsys._h, b"bench", name.encode(), None) == k
        e = fsys.open_file(name, ch)
        assert L.cdc_file_splice_device(e._fh, ch._h, mid, rem, P(fresh.data_ptr()) if ins else None, ins, None,
                                        None) >= 0
        r = delta_leg(label + "_delta", w, e, 0)
        if r["bytes_literal"] > ins or r["ops"] != (3 if ins else 2) or r["bytes_literal_tables"] > 16 * 16384:
            raise SystemExit(f"store_bench: the delta after a 4 KiB edit is not the edit ({label}: {r})")
        delta_leg(label + "_delta_tables_only", w, e, _lib.CDC_DELTA_TABLES_ONLY)
        diff_leg(label + "_diff", w, e)
    r = delta_leg("ak_unrelated_delta", w, o, 0)
    if r["spans_matched"] or r["bytes_copy"] > 64:
        raise SystemExit("store_bench: two unrelated files share bytes")

    def read_plus_verify():
        assert L.cdc_file_read_complete_device(w._fh, P(out.data_ptr()), n, None, P(sp)) == n
        assert L.cdc_file_verify_device(o._fh, P(out.data_ptr()), n, ctypes.byref(first), P(sp)) == 0

    t = timed(read_plus_verify)
    res["ak_unrelated_read_plus_verify"] = {"ms": med(t), "ms_min_max": [min(t), max(t)], "first_diff": first.value}
    diff_leg("ak_unrelated_diff", w, o)

    # (al) the same bytes under other cuts: hardly a slot in common, every byte compared and equal
    ch2 = c.FastChunker(c.SizeParams(2048, 4096, 8192))
    o2 = fsys.create_file("recut", ch2)
    assert L.cdc_file_write_device(o2._fh, ch2._h, P(buf.data_ptr()), n, None) > 0
    r = delta_leg("al_recut_delta", w, o2, 0)
    if r["bytes_literal"] or r["ops"] != 1:
        raise SystemExit(f"store_bench: the delta of equal bytes under other cuts is not one COPY ({r})")
    diff_leg("al_recut_diff", w, o2)
    return res


def pack_legs(a, c, L, P, ch, buf, out, n, k, sp, timed, med):
    """Legs (y)-(ab): the file of (d) packed whole and against a clone after a
    4 KiB overwrite; both packs unpacked into a second layer."""
    import numpy as np
    import torch
    from chunkfs_amd import _lib

    fresh = torch.empty(4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _lib.check(L.cdc_fill_splitmix64_device(P(fresh.data_ptr()), 4096, a.seed + 13, None))
    send = c.FileSystem(store=c.ChunkStore(k + (1 << 14), n + 16 * k + (64 << 20)))
    recv = c.FileSystem(store=c.ChunkStore(k + (1 << 14), n + 16 * k + (64 << 20)))
    w = send.create_file("bench", ch)
    assert L.cdc_file_write_device(w._fh, ch._h, P(buf.data_ptr()), n, None) == k
    st = _lib.cdc_pack_stats_t()
    res = {}
    names = ("pack_sizes", "pack_write", "unpack_header", "unpack_validate", "unpack_hash", "unpack_put",
             "unpack_table")

    def report(name, t, wall, lo, hi):
        split = (ctypes.c_double * 7)()
        assert L.cdc_debug_pack_split(split, 7) == 7
        res[name] = dict({f: getattr(st, f) for f, _ in _lib.cdc_pack_stats_t._fields_ if f != "seconds"},
                         ms=med(t), ms_min_max=[min(t), max(t)], wall_ms=float(np.median(wall)),
                         wall_ms_min_max=[min(wall), max(wall)],
                         GiBps=st.pack_bytes / (1 << 30) / (med(t) * 1e-3),
                         split_ms=dict(zip(names[lo:hi], list(split)[lo:hi])))

    def pack_leg(name, since, pack):
        wall = []

        def call():
            got = L.cdc_file_pack_device(w._fh, since._fh if since else None, None, P(pack.data_ptr()), pack.numel(),
                                         ctypes.byref(st), P(sp))
            assert got == pack.numel(), f"cdc_file_pack_device: {got}"
            wall.append(st.seconds * 1e3)

        t = timed(call)
        report(name, t, wall[a.warmup:], 0, 2)

    def unpack_leg(name, fsys, fname, pack, flags, before):
        wall = []

        def call():
            got = L.cdc_files_unpack_device(fsys._h, fname, P(pack.data_ptr()), pack.numel(),
                                            None if flags else ch._h, flags, ctypes.byref(st), P(sp))
            assert got > 0, f"cdc_files_unpack_device: {got} {L.cdc_last_error()}"
            wall.append(st.seconds * 1e3)

        t = timed(call, before=before)
        report(name, t, wall[a.warmup:], 2, 7)

    def sized(since):
        need = L.cdc_file_pack_device(w._fh, since._fh if since else None, None, None, 0, None, None)
        assert need > 0, f"cdc_file_pack_device: {need}"
        t = torch.empty(need, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        return t

    full = sized(None)
    pack_leg("y_pack_full", None, full)
    unpack_leg("aa_unpack_full_trust", recv, b"bench", full, _lib.CDC_UNPACK_TRUST, recv.clear_database)
    unpack_leg("aa_unpack_full_verified", recv, b"bench", full, 0, recv.clear_database)
    r = recv.open_file_readonly("bench")
    out.zero_()
    assert L.cdc_file_read_complete_device(r._fh, P(out.data_ptr()), n, None, None) == n
    torch.cuda.synchronize()
    if not torch.equal(out, buf) or recv.store.stats() != send.store.stats():
        raise SystemExit("store_bench: the unpacked file or its store is not the sender's")

    assert L.cdc_files_clone(send._h, b"bench", b"base", None) == k
    base = send.open_file_readonly("base")
    assert L.cdc_file_splice_device(w._fh, ch._h, n // 2 + 1234, 4096, P(fresh.data_ptr()), 4096, None, None) >= 0
    inc = sized(base)
    pack_leg("z_pack_after_4k_edit", base, inc)
    assert L.cdc_files_clone(recv._h, b"bench", b"base", None) == k

    def drop():
        if recv.file_exists("v2"):
            recv.remove_file("v2")
            recv.collect()

    unpack_leg("ab_unpack_after_4k_edit", recv, b"v2", inc, 0, drop)
    r2 = recv.open_file_readonly("v2")
    first = ctypes.c_uint64(0)
    assert L.cdc_file_read_complete_device(w._fh, P(out.data_ptr()), n, None, None) == n
    if L.cdc_file_verify_device(r2._fh, P(out.data_ptr()), n, ctypes.byref(first), None) != 1:
        raise SystemExit("store_bench: the file unpacked from the incremental pack is not the edited one")
    return res


def hash_legs(a, c, L, P, ch, buf, n, k, sp, timed, med):
    """Legs (ac)-(ag): both hashers, SHA-256 and BLAKE2sp, side by side in one
    run (DESIGN.md "Hashers").  (ac) hash_ms of a batch of 4 chunks of 16 KiB and
    of one; (ad) the 4 KiB overwrite of (s); (ae) the incremental unpack with the
    check of (ab); (af) the whole write of (d); (ag) the bulk hash over config 3's
    chunk list (bench.py: RabinCDC 2/4/8 KiB over a 256 MiB base and 15 edited
    copies).  Every figure is the median of a.iters calls after a.warmup."""
    import torch
    from chunkfs_amd import _lib
    from chunkfs_amd.synthetic import versioned_archive

    hashers = ("sha256", "blake2sp")
    res = {}

    def both(name, leg):
        r = {h: leg(h) for h in hashers}
        r["sha256_over_blake2sp"] = r["sha256"]["ms"] / r["blake2sp"]["ms"]
        res[name] = r

    def stat(ms, **more):
        return dict(ms=med(ms), ms_min_max=[min(ms), max(ms)], **more)

    # (ac) few chunks: the engine's own hash_ms (order kernels + hash kernel)
    few = torch.tensor([[i * 16384, 16384] for i in range(4)], dtype=torch.int64, device="cuda")
    fdig = torch.empty((4, 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def few_leg(count):
        def leg(h):
            ms = []
            for _ in range(a.warmup + a.iters):
                ch.hash_batch_device([buf.data_ptr()], [0, count], few.data_ptr(), fdig.data_ptr(), hash=h, stream=sp)
                ms.append(ch.last_timing()["hash_ms"])
            return stat(ms[a.warmup:])
        return leg

    both("ac_hash_4x16k", few_leg(4))
    both("ac_hash_1x16k", few_leg(1))

    # (ad) the 4 KiB overwrite in the file of (d), (af) the whole write
    edit = 4096
    fresh = torch.empty(edit * 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _lib.check(L.cdc_fill_splitmix64_device(P(fresh.data_ptr()), fresh.numel(), a.seed + 7, None))

    def overwrite_leg(h):
        fsys = c.FileSystem(store=c.ChunkStore(k + (1 << 14), n + 16 * k + (256 << 20), hash=h))
        w = fsys.create_file("bench", ch)
        assert L.cdc_file_write_device(w._fh, ch._h, P(buf.data_ptr()), n, None) == k
        turn = {"i": 0}

        def call():
            src = fresh.data_ptr() + (turn["i"] % 64) * edit
            turn["i"] += 1
            assert L.cdc_file_splice_device(w._fh, ch._h, n // 2 + 1234, edit, P(src), edit, None, P(sp)) >= 0

        ms = timed(call)
        split = (ctypes.c_double * 5)()
        assert L.cdc_debug_splice_split(split, 5) == 5
        return stat(ms, hash_ms=ch.last_timing()["hash_ms"],
                    split_ms=dict(zip(("planner", "chunk", "resync", "hash_put", "table_build"), split)))

    def write_leg(h):
        fsys = c.FileSystem(store=c.ChunkStore(k, n + 16 * k, hash=h))
        state = {}

        def new_file():
            fsys.clear_database()
            state["w"] = fsys.create_file("bench", ch)

        def call():
            assert L.cdc_file_write_device(state["w"]._fh, ch._h, P(buf.data_ptr()), n, P(sp)) == k

        ms = timed(call, before=new_file)
        return stat(ms, hash_ms=ch.last_timing()["hash_ms"], GiBps=n / (1 << 30) / (med(ms) * 1e-3))

    # (ae) the incremental unpack with the check
    def unpack_leg(h):
        send = c.FileSystem(store=c.ChunkStore(k + (1 << 14), n + 16 * k + (64 << 20), hash=h))
        recv = c.FileSystem(store=c.ChunkStore(k + (1 << 14), n + 16 * k + (64 << 20), hash=h))
        w = send.create_file("bench", ch)
        assert L.cdc_file_write_device(w._fh, ch._h, P(buf.data_ptr()), n, None) == k
        full, _ = send.pack(w)
        recv.unpack("bench", full, trust=True)
        del full
        assert L.cdc_files_clone(send._h, b"bench", b"base", None) == k
        base = send.open_file_readonly("base")
        assert L.cdc_file_splice_device(w._fh, ch._h, n // 2 + 1234, edit, P(fresh.data_ptr()), edit, None, None) >= 0
        inc, pst = send.pack(w, since=base)
        st = _lib.cdc_pack_stats_t()

        def drop():
            if recv.file_exists("v2"):
                recv.remove_file("v2")
                recv.collect()

        def call():
            got = L.cdc_files_unpack_device(recv._h, b"v2", P(inc.data_ptr()), inc.numel(), ch._h, 0,
                                            ctypes.byref(st), P(sp))
            assert got > 0, f"cdc_files_unpack_device: {got} {L.cdc_last_error()}"

        ms = timed(call, before=drop)
        split = (ctypes.c_double * 7)()
        assert L.cdc_debug_pack_split(split, 7) == 7
        return stat(ms, chunks=pst.chunks, chunk_bytes=pst.chunk_bytes, hash_ms=ch.last_timing()["hash_ms"],
                    unpack_hash_ms=split[4])

    both("ad_overwrite_4k", overwrite_leg)
    both("ae_unpack_after_4k_edit", unpack_leg)
    both("af_file_write", write_leg)

    # (ag) the bulk hash: config 3's chunk list, the hashers alternating
    files = versioned_archive(256 << 20, 16)
    bufs = [torch.from_numpy(f).cuda() for f in files]
    lens = [f.size for f in files]
    total = sum(lens)
    rabin = c.RabinChunker(c.SizeParams(2048, 4096, 8192))
    cap = rabin.batch_max_chunks(lens)
    recs = torch.empty((cap, 2), dtype=torch.int64, device="cuda")
    dig = torch.empty((cap, 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ptrs = [b.data_ptr() for b in bufs]
    first = rabin.chunk_batch_device(ptrs, lens, recs.data_ptr(), cap)
    bulk = {h: [] for h in hashers}
    for it in range(a.warmup + a.iters):
        for h in hashers:
            rabin.hash_batch_device(ptrs, first, recs.data_ptr(), dig.data_ptr(), hash=h)
            if it >= a.warmup:
                bulk[h].append(rabin.last_timing()["hash_ms"])
    res["ag_bulk_hash_config3"] = {h: stat(bulk[h], GiBps=total / (1 << 30) / (med(bulk[h]) * 1e-3)) for h in hashers}
    res["ag_bulk_hash_config3"].update(bytes=int(total), chunks=int(first[-1]),
                                       sha256_over_blake2sp=med(bulk["sha256"]) / med(bulk["blake2sp"]))
    # The two conditions of DESIGN.md "Hashers".
    res["condition_few_chunks_3p9x"] = res["ac_hash_4x16k"]["sha256_over_blake2sp"] >= 3.9
    res["condition_bulk_no_slower"] = med(bulk["blake2sp"]) <= max(bulk["sha256"])
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    ap.add_argument("--no-scrub", action="store_true", help="skip the scrub-stage legs (g)-(j)")
    ap.add_argument("--no-batch-write", action="store_true", help="skip the many-files legs (o)-(p)")
    ap.add_argument("--no-collect", action="store_true", help="skip the remove-and-collect legs (q)-(r)")
    ap.add_argument("--no-splice", action="store_true", help="skip the edit-in-place legs (s)-(u)")
    ap.add_argument("--no-snapshot", action="store_true", help="skip the clone and diff legs (v)-(x)")
    ap.add_argument("--no-pack", action="store_true", help="skip the pack and unpack legs (y)-(ab)")
    ap.add_argument("--no-hash", action="store_true", help="skip the two-hasher legs (ac)-(ag)")
    ap.add_argument("--only-hash", action="store_true", help="the two-hasher legs (ac)-(ag) alone")
    ap.add_argument("--no-delta", action="store_true", help="skip the content-aligned delta legs (ah)-(ak)")
    ap.add_argument("--only-delta", action="store_true", help="the content-aligned delta legs (ah)-(ak) alone")
    ap.add_argument("--collect-iters", type=int, default=3)
    ap.add_argument("--scrub-iters", type=int, default=3)
    ap.add_argument("--scrub-groups", default="4096,64m;65536,256m;1048576,1024m",
                    help="RECHUNK groups to time: containers,bytes[k|m] separated by ';'")
    a = ap.parse_args()

    import numpy as np
    import torch
    import chunkfs_amd as c
    from chunkfs_amd import _lib, build

    if not torch.cuda.is_available():
        raise SystemExit("store_bench: no GPU (there is no CPU path to measure)")
    n = a.bytes
    ch = c.FastChunker(c.SizeParams(4096, 8192, 16384))
    buf = torch.empty(n, dtype=torch.uint8, device="cuda")
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    cap = ch.batch_max_chunks([n])
    chunks = torch.empty((cap, 2), dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    sp = s.cuda_stream
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cdc_fill_splitmix64_device(ctypes.c_void_p(buf.data_ptr()), n, a.seed, ctypes.c_void_p(sp)))
    first = ch.chunk_batch_device([buf.data_ptr()], [n], chunks.data_ptr(), cap, stream=sp)
    k = int(first[1])
    dig = torch.empty((k, 32), dtype=torch.uint8, device="cuda")
    found = torch.empty(k, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ch.sha256_batch_device([buf.data_ptr()], first, chunks.data_ptr(), dig.data_ptr(), stream=sp)
    store = c.ChunkStore(k, n + 16 * k)

    hip = _hip_runtime()
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    HIP_MEMCPY_D2D = 3

    def timed(fn, before=None, iters=a.iters, warmup=a.warmup):
        ms = []
        for it in range(warmup + iters):
            if before:
                before()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            fn()
            e1.record(s)
            e1.synchronize()
            if it >= warmup:
                ms.append(e0.elapsed_time(e1))
        return ms

    def finish(res):
        print(json.dumps(res))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")

    if a.only_hash:
        med = lambda v: float(np.median(v))  # noqa: E731
        return finish({"tool": "store_bench", "bytes": n, "chunks": k, "iters": a.iters, "warmup": a.warmup,
                       "device": torch.cuda.get_device_name(0), "source_digest": build.source_digest(),
                       "hash": hash_legs(a, c, _lib.lib(), ctypes.c_void_p, ch, buf, n, k, sp, timed, med)})

    if a.only_delta:
        med = lambda v: float(np.median(v))  # noqa: E731
        return finish({"tool": "store_bench", "bytes": n, "chunks": k, "iters": a.iters, "warmup": a.warmup,
                       "device": torch.cuda.get_device_name(0), "source_digest": build.source_digest(),
                       "delta": delta_legs(a, c, _lib.lib(), ctypes.c_void_p, ch, buf, out, n, k, sp, timed, med)})

    def do_put():
        got = store.put_batch_device([buf.data_ptr()], [n], first, chunks.data_ptr(), dig.data_ptr(), stream=sp)
        assert got == k, "the splitmix64 stream must chunk into unique chunks"

    def do_get():
        assert store.get_device(dig.data_ptr(), k, out.data_ptr(), n, stream=sp) == n

    def do_size():
        assert store.get_device(dig.data_ptr(), k, None, 0, stream=sp) == n

    def do_contains():
        assert store.contains_device(dig.data_ptr(), k, found.data_ptr(), stream=sp) == k

    def do_memcpy():
        rc = hip.hipMemcpyAsync(out.data_ptr(), buf.data_ptr(), n, HIP_MEMCPY_D2D, sp)
        assert rc == 0, f"hipMemcpyAsync: {rc}"

    # The file layer, on a store of its own of the same size.
    L = _lib.lib()
    P = ctypes.c_void_p
    fsys = c.FileSystem(store=c.ChunkStore(k, n + 16 * k))
    state = {}

    def new_file():
        fsys.clear_database()
        state["w"] = fsys.create_file("bench", ch)

    def do_fwrite():
        got = L.cdc_file_write_device(state["w"]._fh, ch._h, P(buf.data_ptr()), n, P(sp))
        assert got == k, f"cdc_file_write_device: {got}"

    def do_fread():
        assert L.cdc_file_read_complete_device(state["w"]._fh, P(out.data_ptr()), n, None, P(sp)) == n

    def do_fsize():
        assert L.cdc_file_read_complete_device(state["w"]._fh, None, 0, None, P(sp)) == n

    def reopen():
        state["r"] = fsys.open_file_readonly("bench")
        state["segments"] = 0

    def do_fsegments():
        fh, total = state["r"]._fh, 0
        while True:
            got = L.cdc_file_read_device(fh, P(out.data_ptr()), c.SEG_SIZE, P(sp))
            assert got >= 0
            if got == 0:
                break
            total += got
            state["segments"] += 1
        assert total == n

    diff = ctypes.c_uint64(0)
    name_buf = ctypes.create_string_buffer(64)
    d_sizes = torch.empty(64, dtype=torch.int64, device="cuda")
    d_counts = torch.empty(64, dtype=torch.int32, device="cuda")

    def do_verify():
        got = L.cdc_file_verify_device(state["w"]._fh, P(buf.data_ptr()), n, ctypes.byref(diff), P(sp))
        assert got == 1, f"cdc_file_verify_device: {got}, first difference at {diff.value}"

    def do_read_then_compare():
        do_fread()
        with torch.cuda.stream(s):
            assert torch.equal(out, buf)

    def do_ratio():
        got = L.cdc_files_get_to_dedup_ratio(fsys._h, b"bench", 4.0, name_buf, 64, P(sp))
        assert got == len(b"bench.4.00") + 1, f"cdc_files_get_to_dedup_ratio: {got}"

    def do_distribution():
        state["bins"] = L.cdc_store_size_distribution_device(fsys.store._h, 1024, P(d_sizes.data_ptr()),
                                                             P(d_counts.data_ptr()), 64, P(sp))
        assert 0 < state["bins"] <= 64, f"cdc_store_size_distribution_device: {state['bins']}"

    t_put = timed(do_put, before=store.clear)
    out.zero_()
    t_get = timed(do_get)
    same = bool(torch.equal(out, buf))  # the file read back is the file written
    t_size = timed(do_size)
    t_contains = timed(do_contains)
    t_memcpy = timed(do_memcpy)
    if not same:
        raise SystemExit("store_bench: get_device did not return the bytes put_batch_device stored")
    t_fwrite = timed(do_fwrite, before=new_file)
    out.zero_()
    t_fread = timed(do_fread)
    fsame = bool(torch.equal(out, buf))
    t_fsize = timed(do_fsize)
    t_fseg = timed(do_fsegments, before=reopen)
    segments = state["segments"]
    t_verify = timed(do_verify)
    t_rcmp = timed(do_read_then_compare)
    out[n // 2 + 12345] ^= 0xFF  # a verify that finds nothing proves nothing: one changed byte must be named
    torch.cuda.synchronize()
    found = L.cdc_file_verify_device(state["w"]._fh, P(out.data_ptr()), n, ctypes.byref(diff), P(sp))
    if found != 0 or diff.value != n // 2 + 12345:
        raise SystemExit(f"store_bench: cdc_file_verify_device missed a changed byte ({found}, {diff.value})")
    t_ratio = timed(do_ratio)
    derived = fsys.stat(fsys.open_file_readonly("bench.4.00"))
    t_dist = timed(do_distribution)
    if int(d_counts[:state["bins"]].sum()) != k:
        raise SystemExit("store_bench: the size distribution does not count every container")
    if not fsame:
        raise SystemExit("store_bench: cdc_file_read_complete_device did not return the bytes written")

    gib = n / (1 << 30)
    med = lambda v: float(np.median(v))  # noqa: E731

    def rate(v):
        return gib / (med(v) * 1e-3)

    copy_ms = med(t_get) - med(t_size)
    res = {
        "tool": "store_bench", "bytes": n, "chunks": k, "iters": a.iters, "warmup": a.warmup,
        "device": torch.cuda.get_device_name(0), "source_digest": build.source_digest(),
        "put_ms": med(t_put), "get_ms": med(t_get), "memcpy_ms": med(t_memcpy),
        "put_ms_min_max": [min(t_put), max(t_put)], "get_ms_min_max": [min(t_get), max(t_get)],
        "memcpy_ms_min_max": [min(t_memcpy), max(t_memcpy)],
        "put_GiBps": rate(t_put), "get_GiBps": rate(t_get), "memcpy_GiBps": rate(t_memcpy),
        "put_vs_memcpy": med(t_memcpy) / med(t_put), "get_vs_memcpy": med(t_memcpy) / med(t_get),
        "contains_ms": med(t_contains), "get_size_only_ms": med(t_size),
        "get_copy_ms": copy_ms, "get_copy_GiBps": gib / (copy_ms * 1e-3) if copy_ms > 0 else None,
        "readback_equal": same,
        # (d) includes chunking and SHA-256, which (a) does not: the two are not compared.
        "file_write_ms": med(t_fwrite), "file_write_ms_min_max": [min(t_fwrite), max(t_fwrite)],
        "file_write_GiBps": rate(t_fwrite),
        "file_read_ms": med(t_fread), "file_read_ms_min_max": [min(t_fread), max(t_fread)],
        "file_read_GiBps": rate(t_fread), "file_read_vs_get": med(t_get) / med(t_fread),
        "file_read_vs_memcpy": med(t_memcpy) / med(t_fread),
        "file_read_size_only_ms": med(t_fsize), "file_read_copy_ms": med(t_fread) - med(t_fsize),
        "file_segments": segments, "file_segment_us": med(t_fseg) * 1e3 / segments,
        "file_segment_pass_ms": med(t_fseg), "file_readback_equal": fsame,
        "verify_ms": med(t_verify), "verify_ms_min_max": [min(t_verify), max(t_verify)],
        "verify_GiBps": rate(t_verify),
        "read_then_compare_ms": med(t_rcmp), "read_then_compare_ms_min_max": [min(t_rcmp), max(t_rcmp)],
        "verify_vs_read_then_compare": med(t_rcmp) / med(t_verify), "verify_vs_file_read": med(t_fread) / med(t_verify),
        "verify_vs_memcpy": med(t_memcpy) / med(t_verify),
        "dedup_ratio4_ms": med(t_ratio), "dedup_ratio4_ms_min_max": [min(t_ratio), max(t_ratio)],
        "dedup_ratio4_spans": derived["spans"], "dedup_ratio4_bytes": derived["size"],
        "size_distribution_ms": med(t_dist), "size_distribution_ms_min_max": [min(t_dist), max(t_dist)],
        "size_distribution_bins": state["bins"],
    }
    if not a.no_scrub:
        res.update(scrub_legs(a, c, L, P, ch, buf, out, n, k, sp, timed, med, med(t_fread)))
    if not a.no_batch_write:
        res["batch_write"] = batch_write_legs(a, c, L, P, ch)
    if not a.no_collect:
        res["collect"] = collect_legs(a, c, L, P, ch, buf, n, med(t_memcpy))
    if not a.no_splice:
        res["splice"] = splice_legs(a, c, L, P, ch, buf, n, k, sp, timed, med)
    if not a.no_snapshot:
        res["snapshot"] = snapshot_legs(a, c, L, P, ch, buf, out, n, k, sp, timed, med)
    if not a.no_pack:
        res["pack"] = pack_legs(a, c, L, P, ch, buf, out, n, k, sp, timed, med)
    if not a.no_hash:
        res["hash"] = hash_legs(a, c, L, P, ch, buf, n, k, sp, timed, med)
    if not a.no_delta:
        res["delta"] = delta_legs(a, c, L, P, ch, buf, out, n, k, sp, timed, med)
    finish(res)


if __name__ == "__main__":
    main()
