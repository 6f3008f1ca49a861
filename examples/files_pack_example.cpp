// files_pack_example.cpp -- replicate a file into a second store through the C++
// mirror (include/chunkfs_amd.hpp, File::pack and Files::unpack): a 1 MiB file is
// written and sent whole; then it is cloned, 4 KiB in the middle are overwritten,
// and the edited file is packed against the clone -- the pack carries only the
// chunks the edit made -- and unpacked into the second store, which holds the
// base.  Both copies read back as the edited bytes.
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
        const size_t len = 1 << 20, patch = 4096, mid = len / 2 + 77;
        std::vector<uint8_t> bytes(len);
        uint32_t x = 2028;
        for (size_t i = 0; i < bytes.size(); ++i) {
            x = x * 1664525u + 1013904223u;
            bytes[i] = (uint8_t)(x >> 24);
        }
        std::vector<uint8_t> want(bytes), edit(patch);
        for (size_t i = 0; i < patch; ++i) want[mid + i] = edit[i] = (uint8_t)~bytes[mid + i];
        uint8_t *d = nullptr, *d_edit = nullptr, *d_back = nullptr, *d_pack = nullptr;
        HIP_OK(hipMalloc((void **)&d, len));
        HIP_OK(hipMalloc((void **)&d_edit, patch));
        HIP_OK(hipMalloc((void **)&d_back, len));
        HIP_OK(hipMemcpy(d, bytes.data(), len, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_edit, edit.data(), patch, hipMemcpyHostToDevice));
        {
            chunkfs_amd::FastChunker chunker({4096, 8192, 16384});
            chunkfs_amd::Store here(1 << 12, 4 << 20), there(1 << 12, 4 << 20);
            chunkfs_amd::Files sender(here), receiver(there);
            chunkfs_amd::File f = sender.create_file("f");
            const int64_t spans = f.write_device(chunker, d, len);

            // The whole file: size the pack, allocate, pack, unpack.  The receiver's store is the sender's.
            cdc_pack_stats_t full{};
            const int64_t full_bytes = f.pack(nullptr, 0, nullptr, nullptr, &full);
            HIP_OK(hipMalloc((void **)&d_pack, (size_t)full_bytes));
            f.pack(d_pack, (size_t)full_bytes);
            const cdc_pack_stats_t got = receiver.unpack("f", d_pack, (size_t)full_bytes, &chunker);
            const cdc_store_stats_t a = here.stats(), b = there.stats();
            if ((int64_t)got.spans != spans || got.chunks_new != full.chunks || std::memcmp(&a, &b, sizeof a)) {
                std::fprintf(stderr, "the receiver's store is not the sender's\n");
                return 1;
            }

            // Snapshot, edit, ship the delta: the pack against the clone carries the new chunks only.
            sender.clone("f", "f.base");
            chunkfs_amd::File base = sender.open_file_readonly("f.base");
            f.pwrite(chunker, mid, d_edit, patch);
            cdc_pack_stats_t delta{};
            const int64_t delta_bytes = f.pack(d_pack, (size_t)full_bytes, &base, nullptr, &delta);
            if (delta.chunks == 0 || delta.chunks > 4 || delta.external_spans + delta.chunks < delta.spans ||
                delta_bytes * 8 > full_bytes) {
                std::fprintf(stderr, "the incremental pack carries %llu chunks in %lld bytes\n",
                             (unsigned long long)delta.chunks, (long long)delta_bytes);
                return 1;
            }
            const cdc_pack_stats_t in = receiver.unpack("f.v2", d_pack, (size_t)delta_bytes, &chunker);

            std::vector<uint8_t> back(len);
            chunkfs_amd::File g = receiver.open_file_readonly("f.v2");
            const int64_t n_read = g.read_complete_device(d_back, len);
            HIP_OK(hipMemcpy(back.data(), d_back, len, hipMemcpyDeviceToHost));
            if (n_read != (int64_t)len || std::memcmp(back.data(), want.data(), len) || in.chunks_new != delta.chunks ||
                in.file_size != len) {
                std::fprintf(stderr, "the received file is not the edited one\n");
                return 1;
            }
            std::printf("pack ok: %lld spans in %lld bytes; the edit in %llu chunks, %lld bytes, %llu spans external\n",
                        (long long)spans, (long long)full_bytes, (unsigned long long)delta.chunks,
                        (long long)delta_bytes, (unsigned long long)delta.external_spans);
        }
        (void)hipFree(d);
        (void)hipFree(d_edit);
        (void)hipFree(d_back);
        (void)hipFree(d_pack);
        return 0;
    } catch (const chunkfs_amd::Error &e) {
        std::fprintf(stderr, "error %d: %s\n", e.code(), e.what());
        return 1;
    }
}
