// files_snapshot_example.cpp -- keep a version of a file through the C++ mirror
// (include/chunkfs_amd.hpp, Files::clone and Files::diff): a 1 MiB file is
// written, cloned, 4 KiB in the middle of the clone are overwritten and the two
// are diffed -- exactly, and from the tables alone.  Then the original is
// removed, a collect drops the containers only it named, and the clone still
// reads back as the edited bytes.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
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
        std::vector<uint8_t> bytes(len);
        uint32_t x = 2027;
        for (size_t i = 0; i < bytes.size(); ++i) {
            x = x * 1664525u + 1013904223u;
            bytes[i] = (uint8_t)(x >> 24);
        }
        std::vector<uint8_t> want(bytes), edit(patch);
        for (size_t i = 0; i < patch; ++i) want[mid + i] = edit[i] = (uint8_t)~bytes[mid + i];  // every byte another
        uint8_t *d = nullptr, *d_edit = nullptr, *d_back = nullptr;
        cdc_chunk_t *d_ranges = nullptr;
        HIP_OK(hipMalloc((void **)&d, len));
        HIP_OK(hipMalloc((void **)&d_edit, patch));
        HIP_OK(hipMalloc((void **)&d_back, len));
        HIP_OK(hipMalloc((void **)&d_ranges, cap * sizeof(cdc_chunk_t)));
        HIP_OK(hipMemcpy(d, bytes.data(), len, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_edit, edit.data(), patch, hipMemcpyHostToDevice));
        {
            chunkfs_amd::FastChunker chunker({4096, 8192, 16384});
            chunkfs_amd::Store store(1 << 12, 4 << 20);
            chunkfs_amd::Files files(store);
            chunkfs_amd::File f = files.create_file("f");
            const int64_t spans = f.write_device(chunker, d, len);
            const uint64_t used = store.stats().arena_used;

            // The snapshot: a table, no data.
            if (files.clone("f", "f.v2") != spans || store.stats().arena_used != used) {
                std::fprintf(stderr, "the clone is no copy of the table alone\n");
                return 1;
            }
            chunkfs_amd::File g = files.open_file("f.v2");
            g.pwrite(chunker, mid, d_edit, patch);

            // What changed: one range, found by reading a few spans of each file.
            const chunkfs_amd::Files::Diff exact = files.diff(f, g, 0, d_ranges, cap);
            cdc_chunk_t r[cap];
            HIP_OK(hipMemcpy(r, d_ranges, sizeof r, hipMemcpyDeviceToHost));
            if (exact.ranges != 1 || r[0].offset != mid || r[0].length != patch ||
                exact.stats.bytes_shared + exact.stats.bytes_compared != len || exact.stats.bytes_compared > 16 * 16384) {
                std::fprintf(stderr, "diff: %lld ranges, the first {%llu, %llu}, %llu bytes compared\n",
                             (long long)exact.ranges, (unsigned long long)r[0].offset, (unsigned long long)r[0].length,
                             (unsigned long long)exact.stats.bytes_compared);
                return 1;
            }
            // The changed spans, with no byte read: a superset.
            const chunkfs_amd::Files::Diff loose = files.diff(f, g, CDC_DIFF_TABLES_ONLY, d_ranges, cap);
            HIP_OK(hipMemcpy(r, d_ranges, sizeof r, hipMemcpyDeviceToHost));
            if (loose.ranges != 1 || loose.stats.bytes_compared != 0 || r[0].offset > mid ||
                r[0].offset + r[0].length < mid + patch || r[0].length != exact.stats.bytes_compared) {
                std::fprintf(stderr, "the tables-only diff does not cover the edit\n");
                return 1;
            }

            // Drop the old version; the clone keeps what it names.
            f.close();
            files.remove("f");
            const cdc_collect_stats_t c = files.collect();
            std::vector<uint8_t> back(len);
            const int64_t n_read = g.read_complete_device(d_back, len);
            HIP_OK(hipMemcpy(back.data(), d_back, len, hipMemcpyDeviceToHost));
            if (n_read != (int64_t)len || std::memcmp(back.data(), want.data(), len) ||
                c.containers_after != g.stat().spans || c.containers_after >= c.containers_before) {
                std::fprintf(stderr, "the clone does not survive the original\n");
                return 1;
            }
            std::printf("snapshot ok: %lld spans cloned; 1 range {%llu, %llu} from %llu bytes compared and %llu shared; "
                        "%llu containers dropped with the original\n",
                        (long long)spans, (unsigned long long)mid, (unsigned long long)patch,
                        (unsigned long long)exact.stats.bytes_compared, (unsigned long long)exact.stats.bytes_shared,
                        (unsigned long long)(c.containers_before - c.containers_after));
        }
        (void)hipFree(d);
        (void)hipFree(d_edit);
        (void)hipFree(d_back);
        (void)hipFree(d_ranges);
        return 0;
    } catch (const chunkfs_amd::Error &e) {
        std::fprintf(stderr, "error %d: %s\n", e.code(), e.what());
        return 1;
    }
}
