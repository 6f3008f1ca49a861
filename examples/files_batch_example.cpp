// files_batch_example.cpp -- many files in one call through the C++ mirror
// (include/chunkfs_amd.hpp, Files::write_batch_device): three files, one of them
// empty and one a copy of the first, written by one batch; a second layer
// receives the same buffers through File::write_device one after another, and
// the two must agree in every file's size and span count and in the store.
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
        const size_t flen = 50000, short_len = 777;
        std::vector<uint8_t> a(flen), back(flen);
        uint32_t x = 2024;
        for (size_t i = 0; i < flen; ++i) {
            x = x * 1664525u + 1013904223u;
            a[i] = (uint8_t)(x >> 24);
        }
        uint8_t *d_a = nullptr, *d_back = nullptr;
        HIP_OK(hipMalloc((void **)&d_a, flen));
        HIP_OK(hipMalloc((void **)&d_back, flen));
        HIP_OK(hipMemcpy(d_a, a.data(), flen, hipMemcpyHostToDevice));
        const char *names[4] = {"a", "empty", "short", "a-again"};
        const uint8_t *datas[4] = {d_a, nullptr, d_a + 4096, d_a};
        const size_t lens[4] = {flen, 0, short_len, flen};
        {
            chunkfs_amd::FastChunker chunker({1024, 2048, 4096});
            chunkfs_amd::Store bstore(1024, 1 << 20), lstore(1024, 1 << 20);
            chunkfs_amd::Files batch(bstore), loop(lstore);
            std::vector<chunkfs_amd::File> bh, lh;
            cdc_fwrite_t reqs[4];
            uint64_t spans[4] = {9, 9, 9, 9};
            for (int i = 0; i < 4; ++i) {
                bh.push_back(batch.create_file(names[i]));
                lh.push_back(loop.create_file(names[i]));
                reqs[i] = cdc_fwrite_t{bh[i].handle(), datas[i], lens[i]};
            }
            const int64_t total = batch.write_batch_device(chunker, 4, reqs, spans);
            int64_t loop_total = 0;
            for (int i = 0; i < 4; ++i) {
                const int64_t got = lh[i].write_device(chunker, datas[i], lens[i]);
                const cdc_file_stat_t sb = bh[i].stat(), sl = lh[i].stat();
                if (got != (int64_t)spans[i] || sb.size != sl.size || sb.spans != sl.spans || sb.size != lens[i]) {
                    std::fprintf(stderr, "file %s: the batch and the loop differ\n", names[i]);
                    return 1;
                }
                loop_total += got;
            }
            const cdc_store_stats_t b = bstore.stats(), l = lstore.stats();
            if (total != loop_total || std::memcmp(&b, &l, sizeof b) || b.index.unique_bytes >= 2 * flen) {
                std::fprintf(stderr, "the stores differ after the batch and the loop\n");
                return 1;
            }
            const int64_t n_read = bh[3].read_complete_device(d_back, flen);
            HIP_OK(hipMemcpy(back.data(), d_back, flen, hipMemcpyDeviceToHost));
            if (n_read != (int64_t)flen || std::memcmp(back.data(), a.data(), flen)) {
                std::fprintf(stderr, "the batch's file reads back differently\n");
                return 1;
            }
            std::printf("batch ok: %zu files, %lld spans, %llu unique chunks\n", batch.list().size(), (long long)total,
                        (unsigned long long)b.index.unique_chunks);
        }
        (void)hipFree(d_a);
        (void)hipFree(d_back);
        return 0;
    } catch (const chunkfs_amd::Error &e) {
        std::fprintf(stderr, "error %d: %s\n", e.code(), e.what());
        return 1;
    }
}
