// Stand-alone driver of the torch-free bucket writer core on host-memory
// columns, for sanitizer builds of the host code (no GPU is touched: host
// batches never reach a HIP call).  Build and run, once per sanitizer:
//
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address \
//       -I hyperspace_amd/csrc tests/native/bucket_writer_check.cpp \
//       hyperspace_amd/csrc/bucket_writer.cpp -o /tmp/bw_asan -lpthread
//   /tmp/bw_asan /tmp/bw_out
//
// and the same with -fsanitize=thread.  It writes small batches at 4 KiB
// and 1-byte-odd chunk sizes with 1, 3 and 15 writer threads, checks size,
// payload offsets and payload bytes of every file, and checks that a
// failing open raises, leaks no fd and leaves the next call working.

#include <dirent.h>
#include <sys/stat.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <vector>

#include "bucket_writer.h"

namespace {

int open_fds() {
  int n = 0;
  DIR* d = opendir("/proc/self/fd");
  if (!d) return -1;
  while (readdir(d)) n++;
  closedir(d);
  return n;
}

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__,    \
                   __LINE__, #cond);                                 \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)

std::string slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  return std::string(std::istreambuf_iterator<char>(f), {});
}

void run_case(const std::string& dir, size_t chunk, int threads) {
  const std::vector<int64_t> rows = {1,    511,  512,  513, 1536, 1792,
                                     1023, 1024, 1025, 3072, 3584, 5};
  int64_t n = 0;
  for (int64_t r : rows) n += r;
  std::vector<int64_t> k(n);
  std::vector<int32_t> a(n);
  std::vector<double> v(n);
  for (int64_t i = 0; i < n; i++) {
    k[i] = i * 7919 - 1000;
    a[i] = (int32_t)(i * 31);
    v[i] = 0.25 * (double)i;
  }
  std::vector<hsw::Column> cols = {
      {k.data(), 8, hsw::T_INT64, "k"},
      {a.data(), 4, hsw::T_INT32, "a"},
      {v.data(), 8, hsw::T_DOUBLE, "v"},
  };
  std::vector<hsw::FileJob> files;
  std::vector<std::pair<std::string, std::string>> stats;
  int64_t lo = 0;
  for (size_t f = 0; f < rows.size(); f++) {
    files.push_back({dir + "/f" + std::to_string(f) + ".parquet", lo,
                     lo + rows[f]});
    for (const hsw::Column& c : cols) {
      const char* p = (const char*)c.base;
      // columns ascend, so first/last row are min/max
      stats.emplace_back(
          std::string(p + lo * c.elem_size, c.elem_size),
          std::string(p + (lo + rows[f] - 1) * c.elem_size, c.elem_size));
    }
    lo += rows[f];
  }
  hsw::Options opt;
  opt.chunk_bytes = chunk;
  opt.writer_threads = threads;
  const int fds = open_fds();
  std::vector<hsw::FileResult> res =
      hsw::write_bucket_files(cols, files, stats, opt);
  CHECK(open_fds() == fds);
  CHECK(res.size() == files.size());
  for (size_t f = 0; f < files.size(); f++) {
    std::string data = slurp(files[f].path);
    struct stat st;
    CHECK(stat(files[f].path.c_str(), &st) == 0);
    CHECK((int64_t)data.size() == res[f].size && st.st_size == res[f].size);
    CHECK(res[f].mtime_ns == (int64_t)st.st_mtim.tv_sec * 1000000000LL +
                                 st.st_mtim.tv_nsec);
    CHECK(data.compare(0, 4, "PAR1") == 0);
    CHECK(data.compare(data.size() - 4, 4, "PAR1") == 0);
    for (size_t c = 0; c < cols.size(); c++) {
      const int64_t nbytes = rows[f] * cols[c].elem_size;
      CHECK(res[f].payload_end[c] - res[f].payload_start[c] == nbytes);
      CHECK(std::memcmp(data.data() + res[f].payload_start[c],
                        (const char*)cols[c].base +
                            files[f].row_lo * cols[c].elem_size,
                        (size_t)nbytes) == 0);
    }
  }

  // a failing open: raises, leaks nothing, and the writer works again
  std::vector<hsw::FileJob> bad = files;
  bad[bad.size() / 2].path = dir + "/f0.parquet/not_a_dir.parquet";
  bool threw = false;
  try {
    hsw::write_bucket_files(cols, bad, stats, opt);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw);
  CHECK(open_fds() == fds);
  res = hsw::write_bucket_files(cols, files, stats, opt);
  CHECK(res.size() == files.size() && open_fds() == fds);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s OUT_DIR\n", argv[0]);
    return 2;
  }
  const std::string dir = argv[1];
  mkdir(dir.c_str(), 0777);
  for (size_t chunk : {(size_t)4096, (size_t)4097, (size_t)1 << 20})
    for (int threads : {1, 3, 15}) run_case(dir, chunk, threads);
  std::printf("bucket_writer_check: ok\n");
  return 0;
}
