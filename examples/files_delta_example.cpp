// files_delta_example.cpp -- what changed between two versions, aligned by content,
// through the C++ mirror (include/chunkfs_amd.hpp, Files::delta): a 1 MiB file is
// written and cloned, 4 KiB are inserted in the middle of the clone, and the delta
// of the two is three ops -- a COPY, the inserted bytes as a LITERAL, and a COPY of
// everything after them from 4 KiB further back.  A diff of the same pair reports
// the whole second half as changed.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <vector>

#include "chunkfs_amd.hpp"

#define HIP_OK(expr)                                                        \
    do {                                                                    \
        hipError_t e_ = (expr);                                             \
        if (e_ != hipSuccess) {                                             \
            std::fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e_)); \
            return 2;                                                       \
        }                                                                   \
    } while (0)

int main() {
    try {
        const size_t len = 1 << 20, patch = 4096, mid = len / 2 + 77, cap = 16;
        std::vector<uint8_t> bytes(len), edit(patch);
        uint32_t x = 2029;
        for (size_t i = 0; i < len + patch; ++i) {
            x = x * 1664525u + 1013904223u;
            (i < len ? bytes[i] : edit[i - len]) = (uint8_t)(x >> 24);
        }
        edit[0] = (uint8_t)~bytes[mid];  // the inserted bytes continue neither neighbour
        edit[patch - 1] = (uint8_t)~bytes[mid - 1];
        uint8_t *d = nullptr, *d_edit = nullptr;
        cdc_delta_op_t *d_ops = nullptr;
        HIP_OK(hipMalloc((void **)&d, len));
        HIP_OK(hipMalloc((void **)&d_edit, patch));
        HIP_OK(hipMalloc((void **)&d_ops, cap * sizeof(cdc_delta_op_t)));
        HIP_OK(hipMemcpy(d, bytes.data(), len, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_edit, edit.data(), patch, hipMemcpyHostToDevice));
        {
            chunkfs_amd::FastChunker chunker({4096, 8192, 16384});
            chunkfs_amd::Store store(1 << 12, 4 << 20);
            chunkfs_amd::Files files(store);
            chunkfs_amd::File f = files.create_file("f");
            f.write_device(chunker, d, len);
            files.clone("f", "f.v2");
            chunkfs_amd::File g = files.open_file("f.v2");
            g.insert(chunker, mid, d_edit, patch);

            const chunkfs_amd::Files::Delta exact = files.delta(f, g, 0, d_ops, cap);
            cdc_delta_op_t op[cap];
            HIP_OK(hipMemcpy(op, d_ops, sizeof op, hipMemcpyDeviceToHost));
            const bool three = exact.ops == 3 && op[0].b_off == 0 && op[0].len == mid && op[0].a_off == 0 &&
                               op[1].b_off == mid && op[1].len == patch && op[1].a_off == CDC_DELTA_LITERAL &&
                               op[2].b_off == mid + patch && op[2].len == len - mid && op[2].a_off == mid;
            if (!three || exact.stats.bytes_literal != patch || exact.stats.bytes_literal_tables > 16 * 16384) {
                std::fprintf(stderr, "delta: %lld ops, %llu literal bytes of %llu after the tables\n",
                             (long long)exact.ops, (unsigned long long)exact.stats.bytes_literal,
                             (unsigned long long)exact.stats.bytes_literal_tables);
                return 1;
            }
            // From the tables alone: the same three ops with whole spans as the LITERAL.
            const chunkfs_amd::Files::Delta loose = files.delta(f, g, CDC_DELTA_TABLES_ONLY);
            // The diff compares position by position: everything after the insert differs.
            const chunkfs_amd::Files::Diff diff = files.diff(f, g);
            if (loose.ops != 3 || loose.stats.bytes_literal != exact.stats.bytes_literal_tables ||
                diff.stats.bytes_differing < len - mid) {
                std::fprintf(stderr, "the tables-only delta or the diff is not what the edit gives\n");
                return 1;
            }
            std::printf("delta ok: 3 ops: COPY {%llu, %llu, %llu}, LITERAL {%llu, %llu}, COPY {%llu, %llu, %llu}; "
                        "%llu bytes read around the edit, the diff calls %llu bytes changed\n",
                        (unsigned long long)op[0].b_off, (unsigned long long)op[0].len, (unsigned long long)op[0].a_off,
                        (unsigned long long)op[1].b_off, (unsigned long long)op[1].len,
                        (unsigned long long)op[2].b_off, (unsigned long long)op[2].len, (unsigned long long)op[2].a_off,
                        (unsigned long long)exact.stats.bytes_literal_tables,
                        (unsigned long long)diff.stats.bytes_differing);
        }
        (void)hipFree(d);
        (void)hipFree(d_edit);
        (void)hipFree(d_ops);
        return 0;
    } catch (const chunkfs_amd::Error &e) {
        std::fprintf(stderr, "error %d: %s\n", e.code(), e.what());
        return 1;
    }
}
