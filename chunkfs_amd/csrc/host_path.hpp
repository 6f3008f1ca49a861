// host_path.hpp -- the host-memory boundary of one chunker handle
// (hostpath.cpp): cdc_chunk_data / cdc_chunk_and_hash on a host buffer and the
// streaming write of one file.
//
// One HostPath = the handle's (Engine::host_).  It owns the pinned upload ring
// with its events and feed words, the copy stream, the host-mapped chunk list,
// the two write windows, the write state and three grow-only device buffers;
// all of it is allocated on first use, so a handle that never touches host
// memory allocates none.
//
// What it uses of its Engine (a friend; nothing else, and no copy of any of it):
//   batch_device       the synchronous batch, with skip_small
//   in_flight, drain_implicit
//   sha256_device
//   max_chunks, algo_, min_, max_, device_
//   own_stream_        every kernel and upload of chunk_host; the windows' chunking
//   fast_              the small path (run_small and its switches), its counters
//   placement()        the handle's one probe
#pragma once
#include <vector>

#include "host_common.hpp"

namespace cdc {

class Engine;

class HostPath {
  public:
    explicit HostPath(Engine &e) : eng_(e) {}
    // With the device current: waits for the copy stream, then frees the ring.
    ~HostPath();

    // chunk_data on a host buffer; with `digests` (32 B per chunk, cap
    // entries) also the SHA-256 of every chunk (StorageWriter's hashing).
    int64_t chunk_host(const uint8_t *data, size_t len, cdc_chunk_t *out, size_t cap, uint8_t *digests = nullptr);
    // ChunkStorage::write of one whole write (storage.rs:78-103, 302-383):
    // the span lengths of the StorageWriter loop over seg_size segments, run
    // through the streaming write path below.
    int64_t fs_write(const uint8_t *data, size_t len, size_t seg_size, std::vector<uint64_t> &spans,
                     double *seconds);
    // Streaming write path: one file write as a sequence of segments
    // (write_from_stream, storage.rs:105-137); spans at finish.
    int write_begin();
    int write_segment(const uint8_t *data, size_t len);
    int64_t write_finish(std::vector<uint64_t> &spans, double *seconds);
    int64_t write_drain(uint64_t *out, size_t cap);
    // Between write_begin and write_finish (cdc_set_gear, cdc_set_rabin_poly:
    // a write never mixes two tables).
    bool write_active() const { return wr_.active; }
    // Host-path statistics: calls, upload s, total s of chunk_host; chunking s
    // and segments of the current / last streaming write; small-kernel calls
    // and fallbacks; the list reader's guard trips.
    int host_stats(double *v, size_t n) const;
    int64_t host_placement_json(char *out, size_t cap);

  private:
    int ensure_ring();
    int ensure_host_out(size_t chunks);
    int ensure_device_data(size_t len);
    int claim_slot(uint32_t &k);  // the next ring slot, once its last DMA or kernel is done
    uint8_t *slot(uint32_t k) const { return static_cast<uint8_t *>(h_ring_) + (size_t)k * kRingSlot; }
    int upload(const uint8_t *src, size_t len, uint8_t *dst, hipStream_t s, size_t piece);
    // The one reader of the host-mapped list: chunks the device buffer d_buf
    // into h_out_, waits for the stream, checks the list; the chunk count.
    // skip_small: the small kernel already declined these bytes.  `who` names
    // the entry point in the refusal.
    int64_t chunk_to_host(const uint8_t *d_buf, size_t len, bool skip_small, const char *who);
    bool tiles(int64_t count, uint64_t len) const;
    int check_list(int64_t count, size_t len, const char *who);
    int write_window(bool final, const char *who);

    Engine &eng_;

    // Pinned upload ring (slot k reused once its event completes; coherent:
    // the small kernel reads a slot while the host fills it).
    static constexpr uint32_t kRingSlots = 4;
    static constexpr size_t kRingSlot = size_t(4) << 20;
    static constexpr size_t kWriteWindow = size_t(256) << 20;
    static constexpr size_t kRingDirect = size_t(16) << 20;  // chunk_data above this: pageable hipMemcpyAsync
    void *h_ring_ = nullptr;
    uint8_t *h_ring_dev_ = nullptr;  // the ring as the device addresses it (small-path kernel reads)
    CopyPool *pool_ = nullptr;       // CopyPool::for_node(the device's node)
    hipEvent_t ring_ev_[kRingSlots] = {};
    uint32_t ring_next_ = 0;
    // Feed words of the small path's streamed input: kFeedPieces per ring
    // slot (pinned, coherent), and their device address.
    uint64_t *h_ready_ = nullptr, *h_ready_dev_ = nullptr;
    // The streaming write's uploads run on the copy stream; copy_done_ makes
    // a window's chunking wait for them, ws_ev_ the next uploads for the carry.
    hipStream_t copy_stream_ = nullptr;
    hipEvent_t copy_done_ = nullptr, ws_ev_ = nullptr;
    // The chunk list the kernels write, host-mapped (pinned through
    // HostPlacement::host_malloc, so a raw pointer), and its device address.
    cdc_chunk_t *h_out_ = nullptr, *d_hout_ = nullptr;
    size_t h_out_cap_ = 0;
    DeviceBuf<uint8_t> ws_win_[2];  // the write's two device windows
    struct WriteState {
        bool active = false, failed = false;
        int cur = 0;
        size_t drained = 0;  // spans already returned by cdc_write_drain
        size_t reserve = 0, carry = 0, fill = 0;
        uint64_t bytes = 0, segments = 0;
        double t0 = 0, chunk_s = 0;
        std::vector<uint64_t> spans;
    } wr_;
    struct HostStats {
        uint64_t calls = 0;
        uint64_t guard_trips = 0;  // chunk lists that did not tile their buffer at first read
        double upload_s = 0, total_s = 0;
    } host_;
    // chunk_host's copy of the caller's bytes; for cdc_chunk_and_hash the
    // chunk list in HBM (the SHA-256 kernel reads it there) and the digests.
    DeviceBuf<uint8_t> d_data_;
    DeviceBuf<cdc_chunk_t> d_out_;
    DeviceBuf<uint8_t> d_dig_;  // 32 bytes per chunk
};

}  // namespace cdc
