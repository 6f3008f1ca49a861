// store_example.cpp -- the device chunk store through the C++ mirror
// (include/chunkfs_amd.hpp, class Store): put three fixed chunks (one a
// duplicate), read two back in another order.  Then the file layer on the same
// store (classes Files and File): write two files from device buffers and read
// one byte range of the second.
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
        std::vector<uint8_t> data(64);
        for (size_t i = 0; i < data.size(); ++i) data[i] = (uint8_t)(i * 37 + 11);
        const cdc_chunk_t chunks[3] = {{0, 10}, {10, 20}, {0, 10}};

        uint8_t *d_data = nullptr, *d_dig = nullptr, *d_new = nullptr, *d_out = nullptr;
        cdc_chunk_t *d_chunks = nullptr, *d_spans = nullptr;
        HIP_OK(hipMalloc((void **)&d_data, data.size()));
        HIP_OK(hipMalloc((void **)&d_dig, 3 * 32));
        HIP_OK(hipMalloc((void **)&d_new, 3));
        HIP_OK(hipMalloc((void **)&d_out, 30));
        HIP_OK(hipMalloc((void **)&d_chunks, sizeof chunks));
        HIP_OK(hipMalloc((void **)&d_spans, 2 * sizeof(cdc_chunk_t)));
        HIP_OK(hipMemcpy(d_data, data.data(), data.size(), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_chunks, chunks, sizeof chunks, hipMemcpyHostToDevice));

        chunkfs_amd::FSChunker hasher(4096);  // any handle hashes chunks
        chunkfs_amd::check(cdc_sha256_chunks_device(hasher.handle(), d_data, d_chunks, 3, d_dig, nullptr));

        chunkfs_amd::Store store(16, 4096);
        const int64_t n_new = store.put_device(d_data, data.size(), d_chunks, d_dig, 3, d_new);
        uint8_t flags[3];
        HIP_OK(hipMemcpy(flags, d_new, 3, hipMemcpyDeviceToHost));
        if (n_new != 2 || flags[0] != 1 || flags[1] != 1 || flags[2] != 0) {
            std::fprintf(stderr, "unexpected new flags\n");
            return 1;
        }
        const cdc_store_stats_t s = store.stats();
        if (s.index.unique_chunks != 2 || s.index.bytes_written != 40 || s.arena_used != 16 + 32) {
            std::fprintf(stderr, "unexpected stats\n");
            return 1;
        }

        // Request order: chunk 1, then chunk 0 (by the digest of its duplicate).
        uint8_t req[64], dig[96];
        HIP_OK(hipMemcpy(dig, d_dig, 96, hipMemcpyDeviceToHost));
        std::memcpy(req, dig + 32, 32);
        std::memcpy(req + 32, dig + 64, 32);
        HIP_OK(hipMemcpy(d_dig, req, 64, hipMemcpyHostToDevice));
        if (store.contains_device(d_dig, 2) != 2) return 1;
        if (store.get_device(d_dig, 2, nullptr, 0) != 30) return 1;
        const int64_t got = store.get_device(d_dig, 2, d_out, 30, d_spans);
        uint8_t out[30];
        cdc_chunk_t spans[2];
        HIP_OK(hipMemcpy(out, d_out, 30, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(spans, d_spans, sizeof spans, hipMemcpyDeviceToHost));
        if (got != 30 || std::memcmp(out, data.data() + 10, 20) || std::memcmp(out + 20, data.data(), 10) ||
            spans[0].offset != 0 || spans[0].length != 20 || spans[1].offset != 20 || spans[1].length != 10) {
            std::fprintf(stderr, "read-back differs\n");
            return 1;
        }
        std::printf("store ok: %lld new of 3, read %lld bytes\n", (long long)n_new, (long long)got);

        // Two files on a store of their own; a range that starts and ends inside chunks.
        const size_t flen = 100000, at = 60000, want = 5000;
        std::vector<uint8_t> a(flen), b(flen), back(want);
        uint32_t x = 12345;
        for (size_t i = 0; i < flen; ++i) {
            x = x * 1664525u + 1013904223u;
            a[i] = (uint8_t)(x >> 24);
            b[i] = (uint8_t)(x >> 16);
        }
        uint8_t *d_a = nullptr, *d_b = nullptr, *d_back = nullptr;
        HIP_OK(hipMalloc((void **)&d_a, flen));
        HIP_OK(hipMalloc((void **)&d_b, flen));
        HIP_OK(hipMalloc((void **)&d_back, want));
        HIP_OK(hipMemcpy(d_a, a.data(), flen, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_b, b.data(), flen, hipMemcpyHostToDevice));
        {
            chunkfs_amd::Store fstore(1024, 1 << 20);
            chunkfs_amd::Files files(fstore);
            chunkfs_amd::FastChunker chunker({1024, 2048, 4096});
            chunkfs_amd::File fa = files.create_file("a"), fb = files.create_file("b");
            const int64_t spans_a = fa.write_device(chunker, d_a, flen);
            const int64_t spans_b = fb.write_device(chunker, d_b, flen);
            fa.close();
            fb.close();
            chunkfs_amd::File rb = files.open_file_readonly("b");
            const int64_t n_read = rb.pread_device(at, want, d_back);
            HIP_OK(hipMemcpy(back.data(), d_back, want, hipMemcpyDeviceToHost));
            if (spans_a < 2 || spans_b < 2 || rb.stat().size != flen || n_read != (int64_t)want ||
                std::memcmp(back.data(), b.data() + at, want) || files.list().size() != 2) {
                std::fprintf(stderr, "file layer read-back differs\n");
                return 1;
            }
            std::printf("files ok: %zu files, pread %lld bytes at %zu\n", files.list().size(), (long long)n_read, at);
        }
        (void)hipFree(d_a);
        (void)hipFree(d_b);
        (void)hipFree(d_back);
        (void)hipFree(d_data);
        (void)hipFree(d_dig);
        (void)hipFree(d_new);
        (void)hipFree(d_out);
        (void)hipFree(d_chunks);
        (void)hipFree(d_spans);
        return 0;
    } catch (const chunkfs_amd::Error &e) {
        std::fprintf(stderr, "error %d: %s\n", e.code(), e.what());
        return 1;
    }
}
