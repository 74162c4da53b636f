// Native writer of the bucketed index files: one call lays out and writes
// every bucket file of a batch as [PAR1][page header + PLAIN payload per
// column][FileMetaData][footer length][PAR1] — REQUIRED numeric columns,
// one row group, one page per column — byte for byte what
// sources/native_parquet.py write_parquet_native produces.
//
// Device batches stream through a pinned ring: one copier thread issues
// chunked D2H copies over two streams, writer threads block on each
// chunk's event and pwrite it at its planned file offset.  Chunks are
// issued round-robin over groups of files, so the writers work on
// different files at any one time.  Host batches pwrite straight from the
// column memory.  No torch types here, so a stand-alone program can drive
// it.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace hsw {

// parquet physical types (parquet.thrift Type)
enum : int { T_INT32 = 1, T_INT64 = 2, T_FLOAT = 4, T_DOUBLE = 5 };

struct Column {
  const void* base;   // first row of the batch (device or host memory)
  int elem_size;      // bytes per value
  int ptype;          // parquet physical type
  std::string name;   // utf-8
};

struct FileJob {
  std::string path;
  int64_t row_lo, row_hi;  // rows [row_lo, row_hi) of every column
};

struct FileResult {
  int64_t size = 0;
  int64_t mtime_ns = 0;
  // per column: file offsets [start, end) of the PLAIN payload
  std::vector<int64_t> payload_start, payload_end;
};

struct Options {
  size_t chunk_bytes = 8u << 20;  // largest single copy / pwrite
  int writer_threads = 15;        // copier + writers <= 16
  bool device_source = false;
  bool timing = false;            // one summary line on stderr
  // device source only: caller-provided pinned ring, split into
  // ring_bytes / chunk_bytes slots; two streams for the copies; both wait
  // on start_event (recorded by the caller after the batch's producer)
  void* ring = nullptr;
  size_t ring_bytes = 0;
  hipStream_t streams[2] = {nullptr, nullptr};
  hipEvent_t start_event = nullptr;
};

// stats[f * ncols + c] = (min bytes, max bytes), PLAIN-encoded.
// Throws std::runtime_error with the first I/O or HIP error; every thread
// is joined and every fd closed before it returns or throws.
std::vector<FileResult> write_bucket_files(
    const std::vector<Column>& cols, const std::vector<FileJob>& files,
    const std::vector<std::pair<std::string, std::string>>& stats,
    const Options& opt);

// The two Thrift pieces, exposed for tests of the encoding.
std::string page_header_bytes(int64_t num_values, int64_t nbytes);

}  // namespace hsw
