// files_collect_example.cpp -- remove, collect and read back through the C++
// mirror (include/chunkfs_amd.hpp, Files::remove / Files::collect): two files
// that share half their bytes fill a small store; the first is removed, the
// collect gives its own chunks' space back, the second file reads back bit for
// bit, and a third file that did not fit before fits now.
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
        const size_t half = 32768, flen = 2 * half;
        std::vector<uint8_t> bytes(4 * half), back(flen);
        uint32_t x = 2025;
        for (size_t i = 0; i < bytes.size(); ++i) {
            x = x * 1664525u + 1013904223u;
            bytes[i] = (uint8_t)(x >> 24);
        }
        uint8_t *d = nullptr, *d_back = nullptr;
        HIP_OK(hipMalloc((void **)&d, bytes.size()));
        HIP_OK(hipMalloc((void **)&d_back, flen));
        HIP_OK(hipMemcpy(d, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
        {
            // Fixed 4 KiB chunks: file "a" = bytes [0, 64 Ki), "b" = [32 Ki, 96 Ki),
            // "c" = [64 Ki, 128 Ki).  The arena holds 140 000 bytes and a put is
            // checked as if every chunk were new: beside a and b (96 Ki unique) c is
            // refused, beside b alone (64 Ki after the collect) it fits.
            chunkfs_amd::FSChunker chunker(4096);
            chunkfs_amd::Store store(64, 140000);
            chunkfs_amd::Files files(store);
            chunkfs_amd::File a = files.create_file("a"), b = files.create_file("b"), c = files.create_file("c");
            a.write_device(chunker, d, flen);
            b.write_device(chunker, d + half, flen);
            try {
                c.write_device(chunker, d + 2 * half, flen);
                std::fprintf(stderr, "the third file should not have fitted\n");
                return 1;
            } catch (const chunkfs_amd::Error &e) {
                if (e.code() != CDC_ENOMEM) throw;
            }
            files.remove("a");
            bool gone = false;
            try {
                a.stat();
            } catch (const chunkfs_amd::Error &e) {
                gone = e.code() == CDC_ENOTFOUND;
            }
            const cdc_collect_stats_t r = files.collect();
            if (!gone || r.containers_before != 24 || r.containers_after != 16 ||
                r.arena_used_before - r.arena_used_after != half || r.bytes_moved != flen) {
                std::fprintf(stderr, "collect: %llu -> %llu containers, %llu -> %llu bytes, %llu moved\n",
                             (unsigned long long)r.containers_before, (unsigned long long)r.containers_after,
                             (unsigned long long)r.arena_used_before, (unsigned long long)r.arena_used_after,
                             (unsigned long long)r.bytes_moved);
                return 1;
            }
            const int64_t n_read = b.read_complete_device(d_back, flen);
            HIP_OK(hipMemcpy(back.data(), d_back, flen, hipMemcpyDeviceToHost));
            if (n_read != (int64_t)flen || std::memcmp(back.data(), bytes.data() + half, flen)) {
                std::fprintf(stderr, "the surviving file reads back differently\n");
                return 1;
            }
            c.write_device(chunker, d + 2 * half, flen);  // fits now: b's second half is shared
            const cdc_store_stats_t s = store.stats();
            std::printf("collect ok: %llu containers kept, %llu bytes moved in %llu + %llu groups, %llu bytes in use\n",
                        (unsigned long long)r.containers_after, (unsigned long long)r.bytes_moved,
                        (unsigned long long)r.groups_direct, (unsigned long long)r.groups_bounced,
                        (unsigned long long)s.arena_used);
        }
        (void)hipFree(d);
        (void)hipFree(d_back);
        return 0;
    } catch (const chunkfs_amd::Error &e) {
        std::fprintf(stderr, "error %d: %s\n", e.code(), e.what());
        return 1;
    }
}
