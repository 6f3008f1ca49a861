// chunkfs_amd.hpp -- header-only C++ mirror of chunkfs's chunking interface,
// built ON the C ABI of chunkfs_amd.h (link with libchunkfs_amd.so).
//
//   reference (Rust, src/lib.rs, src/chunkers)      here
//   struct Chunk {offset, length}   lib.rs:43-66    chunkfs_amd::Chunk
//   trait Chunker                   lib.rs:74-86    chunkfs_amd::Chunker
//   SizeParams {min, avg, max}      chunkers/mod.rs chunkfs_amd::SizeParams
//   FastChunker                     chunkers/fast.rs        chunkfs_amd::FastChunker
//   FSChunker                       chunkers/fixed_size.rs  chunkfs_amd::FSChunker
//   Rabin/Ultra/Leap/SeqChunker     chunkers/{rabin,ultra,leap,seq}.rs  same names
//   (none: this project's own)      --                                  AeChunker, AeMode
//   ChunkStorage::write spans       system/storage.rs:78-103  Chunker::write_spans
//   Database + ChunkStorage::retrieve  system/database.rs, storage.rs:141-157  chunkfs_amd::Store
//   FileSystem / FileLayer / FileHandle  system/mod.rs, file_layer.rs  chunkfs_amd::Files, File
//
// The reference panics on invalid sizes; here constructors throw
// chunkfs_amd::Error (carrying the CDC_E* code and cdc_last_error()).
#pragma once

#include <cstddef>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "chunkfs_amd.h"

namespace chunkfs_amd {

constexpr size_t KB = 1024;
constexpr size_t MB = 1024 * KB;
constexpr size_t GB = 1024 * MB;
constexpr size_t SEG_SIZE = MB;  // src/lib.rs:39

class Error : public std::runtime_error {
  public:
    Error(int code, const std::string &what) : std::runtime_error(what), code_(code) {}
    int code() const { return code_; }

  private:
    int code_;
};

inline int64_t check(int64_t rc) {
    if (rc < 0) throw Error((int)rc, std::string("chunkfs_amd: ") + cdc_last_error());
    return rc;
}

// Chunk (src/lib.rs:41-66): offset and length only.
struct Chunk {
    size_t offset_ = 0;
    size_t length_ = 0;
    Chunk() = default;
    Chunk(size_t offset, size_t length) : offset_(offset), length_(length) {}
    size_t offset() const { return offset_; }
    size_t length() const { return length_; }
    size_t range_begin() const { return offset_; }
    size_t range_end() const { return offset_ + length_; }
    bool operator==(const Chunk &o) const { return offset_ == o.offset_ && length_ == o.length_; }
};

// cdc_chunkers::SizeParams (re-exported at src/chunkers/mod.rs:1).
struct SizeParams {
    size_t min, avg, max;
};

// The Chunker trait (src/lib.rs:74-86).  Not thread-safe: the reference
// serialises every call through Arc<Mutex<dyn Chunker>> (lib.rs:89-90).
class Chunker {
  public:
    virtual ~Chunker() { cdc_destroy(h_); }
    Chunker(const Chunker &) = delete;
    Chunker &operator=(const Chunker &) = delete;

    // chunk_data(&mut self, data, empty) -> Vec<Chunk> (lib.rs:80).
    std::vector<Chunk> chunk_data(const uint8_t *data, size_t len, std::vector<Chunk> empty = {}) {
        std::vector<cdc_chunk_t> raw(cdc_max_chunk_count(h_, len));
        const int64_t n = check(cdc_chunk_data(h_, data, len, raw.data(), raw.size()));
        empty.reserve(empty.size() + (size_t)n);
        for (int64_t i = 0; i < n; ++i) empty.emplace_back(raw[i].offset, raw[i].length);
        return empty;
    }
    std::vector<Chunk> chunk_data(const std::vector<uint8_t> &data, std::vector<Chunk> empty = {}) {
        return chunk_data(data.data(), data.size(), std::move(empty));
    }

    // estimate_chunk_count (lib.rs:85): the reference's own formula.
    size_t estimate_chunk_count(size_t len) const { return cdc_estimate_chunk_count(h_, len); }

    // impl Debug.
    std::string debug() const { return cdc_describe(h_); }

    // ChunkStorage::write + StorageWriter (storage.rs:78-103, 302-383): span
    // lengths of one write call; *chunk_seconds = time inside chunk_data.
    std::vector<uint64_t> write_spans(const uint8_t *data, size_t len, double *chunk_seconds = nullptr,
                                      size_t seg_size = SEG_SIZE) {
        std::vector<uint64_t> spans(cdc_max_chunk_count(h_, len) + 1);
        const int64_t n = check(cdc_fs_write(h_, data, len, seg_size, spans.data(), spans.size(), chunk_seconds));
        spans.resize((size_t)n);
        return spans;
    }

    // ChunkStorage::write_from_stream (storage.rs:105-137) through the
    // streaming write path: begin, one write_segment per StorageWriter::write,
    // finish = flush; returns the span lengths.
    void write_begin() { check(cdc_write_begin(h_)); }
    void write_segment(const uint8_t *data, size_t len) {
        check(cdc_write_segment(h_, data, len));
        written_ += len;
    }
    std::vector<uint64_t> write_finish(double *seconds = nullptr) {
        std::vector<uint64_t> spans(cdc_max_chunk_count(h_, written_) + 1);
        written_ = 0;
        const int64_t n = check(cdc_write_finish(h_, spans.data(), spans.size(), seconds));
        spans.resize((size_t)n);
        return spans;
    }

    // cdc_hash_batch_device: the digests of a batch's chunks with either
    // hasher (CDC_HASH_SHA256 / CDC_HASH_BLAKE2SP).
    void hash_batch_device(int hash, size_t n_streams, const uint8_t *const *d_streams, const uint64_t *first,
                           const cdc_chunk_t *d_chunks, uint8_t *d_digests, void *hip_stream = nullptr) {
        check(cdc_hash_batch_device(h_, hash, n_streams, d_streams, first, d_chunks, d_digests, hip_stream));
    }

    cdc_handle_t *handle() { return h_; }

  protected:
    Chunker() = default;
    Chunker(cdc_algo_t algo, size_t min, size_t avg, size_t max, int device) {
        check(cdc_create(algo, (uint32_t)min, (uint32_t)avg, (uint32_t)max, device, &h_));
    }
    cdc_handle_t *h_ = nullptr;
    size_t written_ = 0;
};

// FastChunker (src/chunkers/fast.rs): FastCDC 2020, default 8/16/64 KiB.
class FastChunker : public Chunker {
  public:
    explicit FastChunker(SizeParams sizes = {8 * KB, 16 * KB, 64 * KB}, int device = 0)
        : Chunker(CDC_ALGO_FASTCDC, sizes.min, sizes.avg, sizes.max, device), sizes_(sizes) {}
    const SizeParams &sizes() const { return sizes_; }

  private:
    SizeParams sizes_;
};

// FSChunker (src/chunkers/fixed_size.rs): fixed size, default 4096.
class FSChunker : public Chunker {
  public:
    explicit FSChunker(size_t chunk_size = 4096, int device = 0)
        : Chunker(CDC_ALGO_FIXED, chunk_size, 0, 0, device), chunk_size_(chunk_size) {}
    size_t chunk_size() const { return chunk_size_; }

  private:
    size_t chunk_size_;
};

// RabinChunker / UltraChunker / LeapChunker (src/chunkers/{rabin,ultra,leap}.rs):
// published algorithms, parity unpinned (cdc-chunkers 0.1.3 absent); sizes are
// explicit because the crate's SizeParams::*_default() values are unknown.
class RabinChunker : public Chunker {
  public:
    explicit RabinChunker(SizeParams sizes, int device = 0)
        : Chunker(CDC_ALGO_RABIN, sizes.min, sizes.avg, sizes.max, device) {}
};

class UltraChunker : public Chunker {
  public:
    explicit UltraChunker(SizeParams sizes, int device = 0)
        : Chunker(CDC_ALGO_ULTRA, sizes.min, sizes.avg, sizes.max, device) {}
};

class LeapChunker : public Chunker {
  public:
    explicit LeapChunker(SizeParams sizes, int device = 0)
        : Chunker(CDC_ALGO_LEAP, sizes.min, sizes.avg, sizes.max, device) {}
};

// seq::OperationMode and seq::Config (re-exported at src/chunkers/seq.rs:3).
enum class OperationMode : uint32_t { Increasing = 0, Decreasing = 1 };
struct SeqConfig {
    uint32_t seq_length = 5, jump_trigger = 50, jump_size = 256;
};

// SeqChunker::new(mode, sizes, config) (src/chunkers/seq.rs:16-24).
class SeqChunker : public Chunker {
  public:
    SeqChunker(OperationMode mode, SizeParams sizes, SeqConfig config = {}, int device = 0) : Chunker() {
        check(cdc_create_seq((uint32_t)mode, config.seq_length, config.jump_trigger, config.jump_size,
                             (uint32_t)sizes.min, (uint32_t)sizes.avg, (uint32_t)sizes.max, device, &h_));
    }
};

// AE, the asymmetric extremum chunker (include/chunkfs_amd.h cdc_create_ae;
// not in the reference).  window 0 = the default for sizes.avg.
enum class AeMode : uint32_t { Max = 0, Min = 1 };

class AeChunker : public Chunker {
  public:
    explicit AeChunker(SizeParams sizes, uint32_t window = 0, AeMode mode = AeMode::Max, int device = 0)
        : Chunker(), window_(window), mode_(mode) {
        if (!window_) {
            const uint64_t w = (uint64_t)sizes.avg * 100000ull / 171828ull;
            window_ = w ? (uint32_t)w : 1u;
        }
        check(cdc_create_ae((uint32_t)mode, window_, (uint32_t)sizes.min, (uint32_t)sizes.avg, (uint32_t)sizes.max,
                            device, &h_));
    }
    uint32_t window() const { return window_; }
    AeMode mode() const { return mode_; }

  private:
    uint32_t window_;
    AeMode mode_;
};

// ChunkerRef (src/lib.rs:89): shared handle to one chunker.
using ChunkerRef = std::shared_ptr<Chunker>;

// Device chunk store: the key -> data Database (system/database.rs:10-36,
// 74-87, first insert wins), ChunkStorage::retrieve (storage.rs:141-157) and
// read_file_complete (system/mod.rs:149-160).  All pointers named d_* are
// DEVICE pointers; a refused call throws and changes nothing.  Not thread-safe.
class Store {
  public:
    Store(size_t max_chunks, size_t arena_bytes, int device = 0, int hash = CDC_HASH_SHA256) {
        check(cdc_store_create(device, max_chunks, arena_bytes, &st_));
        if (hash != CDC_HASH_SHA256 && cdc_store_set_hash(st_, hash) != CDC_OK) {
            cdc_store_destroy(st_);
            check(CDC_EINVAL);
        }
    }
    // The hasher of the store's digests; set_hash only while the store is
    // empty, has no target and is no target.
    void set_hash(int hash) { check(cdc_store_set_hash(st_, hash)); }
    int hash() const { return cdc_store_hash(st_); }
    ~Store() { cdc_store_destroy(st_); }
    Store(const Store &) = delete;
    Store &operator=(const Store &) = delete;

    // Database::insert of n (digest, chunk) pairs; returns the number of new digests.
    int64_t put_device(const uint8_t *d_data, size_t data_len, const cdc_chunk_t *d_chunks, const uint8_t *d_digests,
                       size_t n, uint8_t *d_new = nullptr, void *hip_stream = nullptr) {
        return check(cdc_store_put_device(st_, d_data, data_len, d_chunks, d_digests, n, d_new, hip_stream));
    }
    // The same for the output of cdc_chunk_batch_device + cdc_sha256_batch_device.
    int64_t put_batch_device(size_t n_streams, const uint8_t *const *d_streams, const uint64_t *lens,
                             const uint64_t *first, const cdc_chunk_t *d_chunks, const uint8_t *d_digests,
                             uint8_t *d_new = nullptr, void *hip_stream = nullptr) {
        return check(cdc_store_put_batch_device(st_, n_streams, d_streams, lens, first, d_chunks, d_digests, d_new,
                                                hip_stream));
    }
    // retrieve(..).concat(): total bytes; > out_cap means nothing was written.
    // Throws Error with code CDC_ENOTFOUND if a digest is absent.
    int64_t get_device(const uint8_t *d_digests, size_t n, uint8_t *d_out, size_t out_cap,
                       cdc_chunk_t *d_spans = nullptr, void *hip_stream = nullptr) {
        return check(cdc_store_get_device(st_, d_digests, n, d_out, out_cap, d_spans, hip_stream));
    }
    // Database::contains: how many of the n digests are stored.
    int64_t contains_device(const uint8_t *d_digests, size_t n, uint8_t *d_found = nullptr,
                            void *hip_stream = nullptr) {
        return check(cdc_store_contains_device(st_, d_digests, n, d_found, hip_stream));
    }
    void clear() { check(cdc_store_clear(st_)); }
    // Keeps exactly the containers whose digest is among the n given (duplicates
    // allowed, n = 0 keeps none), drops the rest and compacts the arena in place;
    // returns the number kept.  Throws CDC_ENOTFOUND for a digest that is not
    // stored, CDC_ENOTSUP on a scrubbed store.  Every file layer on the store
    // goes stale (chunkfs_amd.h "Removal and collection").
    int64_t retain_device(const uint8_t *d_digests, size_t n, void *hip_stream = nullptr) {
        return check(cdc_store_retain_device(st_, d_digests, n, hip_stream));
    }
    cdc_store_stats_t stats() const {
        cdc_store_stats_t s{};
        check(cdc_store_stats(st_, &s));
        return s;
    }
    cdc_store_t *handle() { return st_; }

    // Scrub stage (chunkfs_amd.h "Scrub stage"; system/scrub.rs, storage.rs:165-190,
    // 233-235).  `target` becomes this store's target map and must outlive it.
    void set_target(Store &target) { check(cdc_store_set_target(st_, target.st_)); }
    // scrubber: CDC_SCRUB_DUMB / _COPY / _RECHUNK (the last with a chunker on the store's device).
    cdc_scrub_measurements_t scrub(int scrubber, Chunker *chunker = nullptr, void *hip_stream = nullptr) {
        cdc_scrub_measurements_t m{};
        check(cdc_store_scrub(st_, scrubber, chunker ? chunker->handle() : nullptr, &m, hip_stream));
        return m;
    }
    cdc_scrub_stats_t scrub_stats() const {
        cdc_scrub_stats_t s{};
        check(cdc_store_scrub_stats(st_, &s));
        return s;
    }
    // storage_iterator: containers in slot order; d_key_first has cap + 1 entries.
    int64_t iterate_device(uint8_t *d_digests, uint8_t *d_kinds, uint64_t *d_lengths, uint64_t *d_key_first,
                           size_t cap, void *hip_stream = nullptr) {
        return check(cdc_store_iterate_device(st_, d_digests, d_kinds, d_lengths, d_key_first, cap, hip_stream));
    }
    int64_t keys_device(uint8_t *d_keys, size_t cap, void *hip_stream = nullptr) {
        return check(cdc_store_keys_device(st_, d_keys, cap, hip_stream));
    }
    // CDCFixture::size_distribution (bench/mod.rs:218-232): the non-empty bins of
    // length / adjustment * adjustment in ascending order; returns the bin count,
    // > cap means nothing was written.  adjustment == 0 throws (CDC_EINVAL).
    int64_t size_distribution_device(uint64_t adjustment, uint64_t *d_sizes, uint32_t *d_counts, size_t cap,
                                     void *hip_stream = nullptr) {
        return check(cdc_store_size_distribution_device(st_, adjustment, d_sizes, d_counts, cap, hip_stream));
    }

  private:
    cdc_store_t *st_ = nullptr;
};

// FileHandle (file_layer.rs:32-41) on the device file layer: closes on
// destruction.  Move-only.  All pointers named d_* are DEVICE pointers.
class File {
  public:
    File() = default;
    explicit File(cdc_fh_t *fh) : fh_(fh) {}
    ~File() { cdc_file_close(fh_); }
    File(File &&o) noexcept : fh_(o.fh_) { o.fh_ = nullptr; }
    File &operator=(File &&o) noexcept {
        if (this != &o) {
            cdc_file_close(fh_);
            fh_ = o.fh_;
            o.fh_ = nullptr;
        }
        return *this;
    }
    File(const File &) = delete;
    File &operator=(const File &) = delete;

    // write_to_file (mod.rs:93-110) for data in HBM: chunk, SHA-256, put, append.
    int64_t write_device(Chunker &chunker, const uint8_t *d_data, size_t len, void *hip_stream = nullptr) {
        return check(cdc_file_write_device(fh_, chunker.handle(), d_data, len, hip_stream));
    }
    // The same for chunks and digests the caller computed.
    int64_t append_device(const uint8_t *d_data, size_t data_len, const cdc_chunk_t *d_chunks,
                          const uint8_t *d_digests, size_t n, void *hip_stream = nullptr) {
        return check(cdc_file_append_device(fh_, d_data, data_len, d_chunks, d_digests, n, hip_stream));
    }
    // cdc_file_splice_device: the bytes [offset, offset + remove_len) replaced by
    // insert_len bytes from HBM, re-chunked only until the cuts realign.
    cdc_splice_stats_t splice(Chunker &chunker, uint64_t offset, uint64_t remove_len, const uint8_t *d_data,
                              size_t insert_len, void *hip_stream = nullptr) {
        cdc_splice_stats_t s{};
        s.size_before = s.size_after = stat().size;  // what a call with nothing to do leaves unset
        s.resync_offset = offset;
        check(cdc_file_splice_device(fh_, chunker.handle(), offset, remove_len, d_data, insert_len, &s, hip_stream));
        return s;
    }
    // Overwrite up to the end of the file and extend past it, as pwrite(2).
    cdc_splice_stats_t pwrite(Chunker &chunker, uint64_t offset, const uint8_t *d_data, size_t len,
                              void *hip_stream = nullptr) {
        const uint64_t size = stat().size, left = offset < size ? size - offset : 0;
        return splice(chunker, offset, len < left ? len : left, d_data, len, hip_stream);
    }
    cdc_splice_stats_t insert(Chunker &chunker, uint64_t offset, const uint8_t *d_data, size_t len,
                              void *hip_stream = nullptr) {
        return splice(chunker, offset, 0, d_data, len, hip_stream);
    }
    cdc_splice_stats_t delete_range(Chunker &chunker, uint64_t offset, uint64_t len, void *hip_stream = nullptr) {
        return splice(chunker, offset, len, nullptr, 0, hip_stream);
    }
    // A size above the file's is refused (CDC_EINVAL: offset past the end).
    cdc_splice_stats_t truncate(Chunker &chunker, uint64_t size, void *hip_stream = nullptr) {
        const uint64_t have = stat().size;
        return splice(chunker, size, size < have ? have - size : 0, nullptr, 0, hip_stream);
    }
    // read_file_complete (mod.rs:149-152): the size; > out_cap means nothing was written.
    int64_t read_complete_device(uint8_t *d_out, size_t out_cap, cdc_chunk_t *d_spans = nullptr,
                                 void *hip_stream = nullptr) {
        return check(cdc_file_read_complete_device(fh_, d_out, out_cap, d_spans, hip_stream));
    }
    // read_from_file (mod.rs:157-160): one segment of whole spans from the cursor.
    int64_t read_device(uint8_t *d_out, size_t out_cap, void *hip_stream = nullptr) {
        return check(cdc_file_read_device(fh_, d_out, out_cap, hip_stream));
    }
    // The bytes [offset, min(offset + len, size)).
    int64_t pread_device(uint64_t offset, size_t len, uint8_t *d_out, void *hip_stream = nullptr) {
        return check(cdc_file_pread_device(fh_, offset, len, d_out, hip_stream));
    }
    // FileLayer::read_complete (file_layer.rs:127-133): the span digests.
    int64_t hashes_device(uint8_t *d_digests, size_t cap) { return check(cdc_file_hashes_device(fh_, d_digests, cap)); }
    // chunk_count_distribution (file_layer.rs:188-206), first-occurrence order.
    int64_t distribution_device(uint8_t *d_digests, uint32_t *d_counts, uint64_t *d_lengths, size_t cap,
                                void *hip_stream = nullptr) {
        return check(cdc_file_distribution_device(fh_, d_digests, d_counts, d_lengths, cap, hip_stream));
    }
    // CDCFixture::verify (bench/mod.rs:241-275) without the read-back: true when
    // the file equals d_data[0..len); *first_diff (nullable) = the smallest
    // differing offset, min(size, len) when only the sizes differ, ~0 when equal.
    bool verify_device(const uint8_t *d_data, size_t len, uint64_t *first_diff = nullptr,
                       void *hip_stream = nullptr) {
        return check(cdc_file_verify_device(fh_, d_data, len, first_diff, hip_stream)) != 0;
    }
    // cdc_file_pack_device: the file as a pack in d_pack (DEVICE, 16-byte aligned,
    // cap bytes).  Chunks that a span of `since` (nullable) names, or a span i with
    // d_have[i] != 0 (nullable, DEVICE u8[spans]), are left out.  Returns the
    // pack's size: nothing was written when it exceeds cap, and cap = 0 sizes a
    // pack.  stats (nullable) is filled either way.
    int64_t pack(uint8_t *d_pack, size_t cap, File *since = nullptr, const uint8_t *d_have = nullptr,
                 cdc_pack_stats_t *stats = nullptr, void *hip_stream = nullptr) {
        return check(cdc_file_pack_device(fh_, since ? since->fh_ : nullptr, d_have, d_pack, cap, stats, hip_stream));
    }
    cdc_file_stat_t stat() const {
        cdc_file_stat_t s{};
        check(cdc_file_stat(fh_, &s));
        return s;
    }
    // close_file (mod.rs:140-146); stat() first for the measurements.
    void close() {
        cdc_file_close(fh_);
        fh_ = nullptr;
    }
    cdc_fh_t *handle() { return fh_; }

  private:
    cdc_fh_t *fh_ = nullptr;
};

// The device file layer over one Store: FileSystem's file calls
// (system/mod.rs:58-160, 271-278).  A span's offset is its true byte position
// in the file (the one deviation from file_layer.rs:136-145).  The Store must
// outlive the Files; a refused call throws and changes nothing.
class Files {
  public:
    explicit Files(Store &store, size_t seg_size = SEG_SIZE) { check(cdc_files_create(store.handle(), seg_size, &fs_)); }
    ~Files() { cdc_files_destroy(fs_); }
    Files(const Files &) = delete;
    Files &operator=(const Files &) = delete;

    // FileLayer::create (file_layer.rs:84-99); create_file passes create_new = true.
    File create(const std::string &name, bool create_new) {
        cdc_fh_t *fh = nullptr;
        check(cdc_files_create_file(fs_, name.c_str(), create_new ? 1 : 0, &fh));
        return File(fh);
    }
    File create_file(const std::string &name) { return create(name, true); }
    File open_file(const std::string &name) { return open(name, false); }
    File open_file_readonly(const std::string &name) { return open(name, true); }
    bool exists(const std::string &name) const { return check(cdc_files_exists(fs_, name.c_str())) != 0; }
    std::vector<std::string> list() const {
        std::vector<char> buf((size_t)check(cdc_files_list(fs_, nullptr, 0)));
        check(cdc_files_list(fs_, buf.data(), buf.size()));
        std::vector<std::string> names;
        for (size_t at = 0; at < buf.size(); at += names.back().size() + 1) names.emplace_back(buf.data() + at);
        return names;
    }
    // Many ranges over many files, planned and copied as one piece list.
    void pread_batch_device(size_t n, const cdc_pread_t *reqs, uint64_t *got, void *hip_stream = nullptr) {
        check(cdc_files_pread_batch_device(fs_, n, reqs, got, hip_stream));
    }
    // n write_to_file calls as one (cdc_files_write_batch_device): one chunk
    // batch, one hash batch, one put, one append; the files and the store end
    // up as the n single writes in request order would leave them.  spans
    // (nullable, n entries) receives each request's count; returns their sum.
    int64_t write_batch_device(Chunker &chunker, size_t n, const cdc_fwrite_t *reqs, uint64_t *spans = nullptr,
                               void *hip_stream = nullptr) {
        return check(cdc_files_write_batch_device(fs_, chunker.handle(), n, reqs, spans, hip_stream));
    }
    // get_to_dedup_ratio (mod.rs:170-178, file_layer.rs:208-268): derives the file
    // "{name}.{ratio:.2}" and returns its name; span offsets in it are true byte
    // positions.  Throws CDC_EINVAL for a ratio < 1, NaN or infinite, and when the
    // repeating spans are all empty.
    std::string get_to_dedup_ratio(const std::string &name, double dedup_ratio, void *hip_stream = nullptr) {
        std::vector<char> buf(name.size() + 400);
        check(cdc_files_get_to_dedup_ratio(fs_, name.c_str(), dedup_ratio, buf.data(), buf.size(), hip_stream));
        return std::string(buf.data());
    }
    // Drops the file (host only); throws CDC_ENOTFOUND for an unknown name.  Calls
    // through handles to it throw CDC_ENOTFOUND from here on.
    void remove(const std::string &name) { check(cdc_files_remove(fs_, name.c_str())); }
    // Keeps exactly the containers some file of this layer references, compacts
    // the arena in place and rewrites every file's table (chunkfs_amd.h "Removal
    // and collection").  A second layer on the same store goes stale.
    cdc_collect_stats_t collect(void *hip_stream = nullptr) {
        cdc_collect_stats_t s{};
        check(cdc_files_collect(fs_, &s, hip_stream));
        return s;
    }
    // cdc_files_clone: the new file `dst` with a deep copy of src's span table; no
    // put, no arena byte moved.  Returns the span count.  Throws CDC_ENOTFOUND
    // for an unknown or stale src, CDC_EEXIST when dst exists.
    int64_t clone(const std::string &src, const std::string &dst, void *hip_stream = nullptr) {
        return check(cdc_files_clone(fs_, src.c_str(), dst.c_str(), hip_stream));
    }
    // cdc_files_diff_device: where two files differ, as maximal runs {offset,
    // length} in d_ranges (DEVICE, cap entries; written only when the count is <=
    // cap), and the stats.  Shared pieces are not read; CDC_DIFF_TABLES_ONLY
    // reads no data at all.
    struct Diff {
        int64_t ranges;
        cdc_diff_stats_t stats;
    };
    Diff diff(File &a, File &b, uint32_t flags = 0, cdc_chunk_t *d_ranges = nullptr, size_t cap = 0,
              void *hip_stream = nullptr) {
        Diff d{};
        d.ranges = check(cdc_files_diff_device(a.handle(), b.handle(), flags, d_ranges, cap, &d.stats, hip_stream));
        return d;
    }
    // cdc_files_delta_device: the edit script that builds b (new) out of a (old),
    // aligned by content: COPY {b_off, len, a_off} and LITERAL {b_off, len,
    // CDC_DELTA_LITERAL} ops that tile [0, size_b), in d_ops (DEVICE, cap entries;
    // written only when the count is <= cap), and the stats.
    // CDC_DELTA_TABLES_ONLY reads no data: whole unmatched spans are LITERAL.
    struct Delta {
        int64_t ops;
        cdc_delta_stats_t stats;
    };
    Delta delta(File &a, File &b, uint32_t flags = 0, cdc_delta_op_t *d_ops = nullptr, size_t cap = 0,
                void *hip_stream = nullptr) {
        Delta d{};
        d.ops = check(cdc_files_delta_device(a.handle(), b.handle(), flags, d_ops, cap, &d.stats, hip_stream));
        return d;
    }
    // cdc_files_unpack_device: the new file `name` from the len bytes of a pack at
    // d_pack (DEVICE, 16-byte aligned).  The pack is validated before anything is
    // written; hasher (nullable only with CDC_UNPACK_TRUST) checks the carried
    // chunks against their digests.  Throws CDC_EINVAL naming the failed check,
    // CDC_ENOTFOUND for an external span whose chunk the store lacks, CDC_EEXIST,
    // CDC_ENOMEM.  Returns the stats; stats.spans is the new file's span count.
    cdc_pack_stats_t unpack(const std::string &name, const uint8_t *d_pack, size_t len, Chunker *hasher,
                            uint32_t flags = 0, void *hip_stream = nullptr) {
        cdc_pack_stats_t s{};
        check(cdc_files_unpack_device(fs_, name.c_str(), d_pack, len, hasher ? hasher->handle() : nullptr, flags, &s,
                                      hip_stream));
        return s;
    }
    // clear_database (mod.rs:275-278): no files, an empty store, handles invalid.
    void clear() { check(cdc_files_clear(fs_)); }
    // clear_file_system (mod.rs:294-297): the target map first, so that the
    // store's clear adopts the emptied target.
    void clear_file_system(Store &target) {
        target.clear();
        clear();
    }
    cdc_files_t *handle() { return fs_; }

  private:
    File open(const std::string &name, bool readonly) {
        cdc_fh_t *fh = nullptr;
        check(cdc_files_open(fs_, name.c_str(), readonly ? 1 : 0, &fh));
        return File(fh);
    }
    cdc_files_t *fs_ = nullptr;
};

}  // namespace chunkfs_amd
