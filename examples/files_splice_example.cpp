// files_splice_example.cpp -- edit a file in place through the C++ mirror
// (include/chunkfs_amd.hpp, File::splice and its thin forms): a 1 MiB file is
// written once, 4 KiB in its middle are overwritten, 100 bytes inserted and 100
// other bytes deleted.  Each edit re-chunks a few spans only; the file reads back
// as the edited bytes and a collect drops the replaced spans' containers.
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
        const size_t len = 1 << 20, patch = 4096, mid = len / 2;
        std::vector<uint8_t> bytes(len + patch + 100);
        uint32_t x = 2026;
        for (size_t i = 0; i < bytes.size(); ++i) {
            x = x * 1664525u + 1013904223u;
            bytes[i] = (uint8_t)(x >> 24);
        }
        uint8_t *d = nullptr, *d_back = nullptr;
        HIP_OK(hipMalloc((void **)&d, bytes.size()));
        HIP_OK(hipMalloc((void **)&d_back, len + 100));
        HIP_OK(hipMemcpy(d, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
        {
            chunkfs_amd::FastChunker chunker({4096, 8192, 16384});
            chunkfs_amd::Store store(1 << 12, 4 << 20);
            chunkfs_amd::Files files(store);
            chunkfs_amd::File f = files.create_file("f");
            const int64_t spans = f.write_device(chunker, d, len);

            // The expected bytes, edited on the host the same way.
            std::vector<uint8_t> want(bytes.begin(), bytes.begin() + len);
            const cdc_splice_stats_t w = f.pwrite(chunker, mid, d + len, patch);
            std::memcpy(want.data() + mid, bytes.data() + len, patch);
            const cdc_splice_stats_t i = f.insert(chunker, 1000, d + len + patch, 100);
            want.insert(want.begin() + 1000, bytes.begin() + len + patch, bytes.begin() + len + patch + 100);
            const cdc_splice_stats_t r = f.delete_range(chunker, 900000, 100);
            want.erase(want.begin() + 900000, want.begin() + 900100);

            std::vector<uint8_t> back(want.size());
            const int64_t n_read = f.read_complete_device(d_back, len + 100);
            HIP_OK(hipMemcpy(back.data(), d_back, back.size(), hipMemcpyDeviceToHost));
            if (n_read != (int64_t)want.size() || std::memcmp(back.data(), want.data(), want.size())) {
                std::fprintf(stderr, "the edited file reads back differently\n");
                return 1;
            }
            const cdc_splice_stats_t *all[3] = {&w, &i, &r};
            for (const cdc_splice_stats_t *s : all)
                if (s->rounds != 1 || s->spans_removed > 8 || s->window_bytes > 200000) {
                    std::fprintf(stderr, "an edit re-chunked more than its neighbourhood: %llu spans, %llu bytes\n",
                                 (unsigned long long)s->spans_removed, (unsigned long long)s->window_bytes);
                    return 1;
                }
            const cdc_collect_stats_t g = files.collect();
            if (g.containers_after != f.stat().spans || g.containers_after >= g.containers_before) {
                std::fprintf(stderr, "collect kept %llu containers for %llu spans\n",
                             (unsigned long long)g.containers_after, (unsigned long long)f.stat().spans);
                return 1;
            }
            std::printf("splice ok: %lld spans written; overwrite -%llu +%llu spans over %llu bytes, insert -%llu +%llu, "
                        "delete -%llu +%llu; %llu containers dropped by the collect\n",
                        (long long)spans, (unsigned long long)w.spans_removed, (unsigned long long)w.spans_inserted,
                        (unsigned long long)w.window_bytes, (unsigned long long)i.spans_removed,
                        (unsigned long long)i.spans_inserted, (unsigned long long)r.spans_removed,
                        (unsigned long long)r.spans_inserted,
                        (unsigned long long)(g.containers_before - g.containers_after));
        }
        (void)hipFree(d);
        (void)hipFree(d_back);
        return 0;
    } catch (const chunkfs_amd::Error &e) {
        std::fprintf(stderr, "error %d: %s\n", e.code(), e.what());
        return 1;
    }
}
