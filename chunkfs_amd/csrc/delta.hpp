// delta.hpp -- the device path of cdc_files_delta_device (delta.hip) and what its
// host side (files_host.cpp) sizes for it.  The arithmetic: delta_plan.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "files.hpp"

namespace cdc {

// One op of the edit script: cdc_delta_op_t.
struct DeltaOp {
    uint64_t b_off, len, a_off;
};

// Device scratch for two tables of na and nb > 0 spans; every size is a bound
// the host has before the first launch.
struct DeltaScratch {
    uint64_t *key_in, *key;   // [na] A's slots, before and after the sort
    uint32_t *idx_in, *idx;   // [na] A's span indices, likewise
    void *sort_tmp;           // rocPRIM's scratch, sort_bytes of it
    size_t sort_bytes;
    int64_t *diag;            // [nb] per span of B: its diagonal, kDeltaNone or kDeltaSkip
    uint64_t *rflag;          // [nb] the span begins a run; scanned
    uint64_t *rb;             // [nb + 1] the runs: first byte in B, closed by size_b
    int64_t *rd;              // [nb + 1] their diagonal, kDeltaNone for a LITERAL run
    uint64_t *tstart;         // [nb] tiles per run (0 for a COPY run); scanned
    unsigned long long *fwd;  // [nb] per region: the forward match so far, preset to its cap
    unsigned long long *bwd;  // [nb] per region: the lowest x from which the backward match holds, preset to its floor
    uint64_t *hcount;         // [nb] ops a run opens; scanned
    uint64_t *hb, *ha;        // [3 nb] the ops in order: b_off and a_off
    uint64_t *bs_r, *bs_t, *bs_h;  // block sums of the three scans: store_scan_blocks(nb) + 1 each
    const uint64_t *n_runs, *n_tiles, *n_ops;  // their totals
    unsigned long long *acc;  // [4] bytes_literal, bytes_literal_tables, spans_matched, regions
    uint64_t max_tiles;       // size_b / kDeltaTile + nb
};

// The whole device path, no host wait inside.  Both files hold bytes.  h_out
// (pinned): [0] ops, [1] bytes_copy, [2] bytes_literal, [3] bytes_literal_tables,
// [4] spans_matched, [5] regions.  d_ops receives the ops when their number is
// <= cap, and is left alone otherwise.
hipError_t launch_files_delta(const DiffSide &a, const DiffSide &b, uint64_t arena, bool tables_only,
                              const DeltaScratch &w, DeltaOp *d_ops, uint64_t cap, unsigned long long *h_out,
                              hipStream_t s);

}  // namespace cdc
