// Native bucketed-index file writer — see bucket_writer.h.
//
// The Thrift compact encoding below is a port of TWriter /
// write_parquet_native in sources/native_parquet.py for the one shape the
// index build writes; the Python writer stays the reference and the tests
// compare the two byte for byte.

#include "bucket_writer.h"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <thread>

namespace hsw {
namespace {

// Thrift compact type ids
enum : int { CT_I32 = 5, CT_I64 = 6, CT_BINARY = 8, CT_LIST = 9,
             CT_STRUCT = 12 };

class TWriter {
 public:
  std::string buf;

  void struct_begin() { last_.push_back(0); }
  void struct_end() {
    buf.push_back('\0');
    last_.pop_back();
  }
  void field_i32(int fid, int64_t v) {
    field(fid, CT_I32);
    varint(zigzag(v));
  }
  void field_i64(int fid, int64_t v) {
    field(fid, CT_I64);
    varint(zigzag(v));
  }
  void field_binary(int fid, const std::string& s) {
    field(fid, CT_BINARY);
    binary(s);
  }
  void field_list_begin(int fid, int etype, size_t size) {
    field(fid, CT_LIST);
    if (size < 15) {
      buf.push_back((char)((size << 4) | etype));
    } else {
      buf.push_back((char)(0xF0 | etype));
      varint(size);
    }
  }
  void field_struct_begin(int fid) {
    field(fid, CT_STRUCT);
    struct_begin();
  }
  void i32_elem(int64_t v) { varint(zigzag(v)); }
  void binary(const std::string& s) {
    varint(s.size());
    buf += s;
  }

 private:
  std::vector<int> last_{0};

  static uint64_t zigzag(int64_t n) {
    return ((uint64_t)n << 1) ^ (uint64_t)(n >> 63);
  }
  void varint(uint64_t n) {
    while (true) {
      uint8_t b = n & 0x7F;
      n >>= 7;
      if (n) {
        buf.push_back((char)(b | 0x80));
      } else {
        buf.push_back((char)b);
        return;
      }
    }
  }
  void field(int fid, int ctype) {
    int delta = fid - last_.back();
    if (delta > 0 && delta <= 15) {
      buf.push_back((char)((delta << 4) | ctype));
    } else {
      buf.push_back((char)ctype);
      varint(zigzag(fid));
    }
    last_.back() = fid;
  }
};

struct ColMeta {
  int64_t off;     // page header offset in the file
  int64_t nbytes;  // page header + payload
};

std::string footer_bytes(const std::vector<Column>& cols,
                         const std::vector<ColMeta>& meta, int64_t num_rows,
                         const std::pair<std::string, std::string>* stats) {
  TWriter w;
  w.struct_begin();
  w.field_i32(1, 2);  // version
  w.field_list_begin(2, CT_STRUCT, 1 + cols.size());
  w.struct_begin();  // schema root
  w.field_binary(4, "schema");
  w.field_i32(5, (int64_t)cols.size());
  w.struct_end();
  for (const Column& c : cols) {
    w.struct_begin();
    w.field_i32(1, c.ptype);
    w.field_i32(3, 0);  // REQUIRED
    w.field_binary(4, c.name);
    w.struct_end();
  }
  w.field_i64(3, num_rows);
  w.field_list_begin(4, CT_STRUCT, 1);  // row_groups
  w.struct_begin();
  int64_t total_bytes = 0;
  w.field_list_begin(1, CT_STRUCT, cols.size());
  for (size_t c = 0; c < cols.size(); c++) {
    total_bytes += meta[c].nbytes;
    const std::string& mn = stats[c].first;
    const std::string& mx = stats[c].second;
    w.struct_begin();  // ColumnChunk
    w.field_i64(2, meta[c].off);
    w.field_struct_begin(3);  // ColumnMetaData
    w.field_i32(1, cols[c].ptype);
    w.field_list_begin(2, CT_I32, 1);
    w.i32_elem(0);  // PLAIN
    w.field_list_begin(3, CT_BINARY, 1);
    w.binary(cols[c].name);
    w.field_i32(4, 0);  // UNCOMPRESSED
    w.field_i64(5, num_rows);
    w.field_i64(6, meta[c].nbytes);
    w.field_i64(7, meta[c].nbytes);
    w.field_i64(9, meta[c].off);  // data_page_offset
    if (!mn.empty()) {
      w.field_struct_begin(12);  // Statistics
      w.field_binary(1, mx);     // max (legacy)
      w.field_binary(2, mn);     // min (legacy)
      w.field_i64(3, 0);         // null_count
      w.field_binary(5, mx);     // max_value
      w.field_binary(6, mn);     // min_value
      w.struct_end();
    }
    w.struct_end();
    w.struct_end();
  }
  w.field_i64(2, total_bytes);
  w.field_i64(3, num_rows);
  w.struct_end();
  w.field_binary(6, "hyperspace_amd 0.1");
  w.struct_end();
  return std::move(w.buf);
}

// One file: every small piece (magic, page headers, footer) is known
// before any payload moves, and so is every payload offset.
struct FilePlan {
  std::vector<std::pair<int64_t, std::string>> pieces;  // (offset, bytes)
  std::mutex open_mu;
  bool open_tried = false;
  int fd = -1;
  std::atomic<int64_t> remaining{0};  // payload chunks not yet written
};

struct Task {
  int file;
  int64_t file_off;
  const char* src;
  size_t nbytes;
};

constexpr size_t kFileGroup = 16;

int64_t now_ns() {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(
             std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

struct Issued {
  size_t task;
  int slot;
};

class Run {
 public:
  Run(const std::vector<FileJob>& files, const Options& opt,
      std::vector<FileResult>& results)
      : files_(files), opt_(opt), results_(results),
        plans_(new FilePlan[files.size()]) {}

  FilePlan* plans() { return plans_.get(); }
  std::vector<Task> tasks;

  void fail(const std::string& what) {
    std::lock_guard<std::mutex> g(err_mu_);
    if (!failed_.load()) {
      error_ = what;
      failed_.store(true);
    }
  }
  bool failed() const { return failed_.load(); }
  const std::string& error() const { return error_; }

  // ---- host source: writers pull tasks off a counter -------------------
  void host_writer() {
    while (!failed()) {
      size_t i = next_.fetch_add(1);
      if (i >= tasks.size()) return;
      const int64_t t0 = now_ns();
      write_task(tasks[i], tasks[i].src);
      ns_write_ += now_ns() - t0;
    }
  }

  // ---- device source ---------------------------------------------------
  void init_ring(int nslots, hipEvent_t* events) {
    events_ = events;
    for (int s = nslots - 1; s >= 0; s--) free_.push_back(s);
  }

  // the copier runs on the calling thread
  void copier() {
    for (int s = 0; s < 2 && !failed(); s++)
      hip(hipStreamWaitEvent(opt_.streams[s], opt_.start_event, 0),
          "hipStreamWaitEvent");
    for (size_t i = 0; i < tasks.size() && !failed(); i++) {
      int slot;
      {
        const int64_t t0 = now_ns();
        std::unique_lock<std::mutex> g(mu_);
        cv_free_.wait(g, [&] { return !free_.empty(); });
        slot = free_.back();
        free_.pop_back();
        ns_slot_wait_ += now_ns() - t0;
      }
      hipStream_t st = opt_.streams[i & 1];
      char* dst = (char*)opt_.ring + (size_t)slot * opt_.chunk_bytes;
      bool ok = !failed() &&
                hip(hipMemcpyAsync(dst, tasks[i].src, tasks[i].nbytes,
                                   hipMemcpyDeviceToHost, st),
                    "hipMemcpyAsync");
      if (ok && !hip(hipEventRecord(events_[slot], st), "hipEventRecord")) {
        (void)hipStreamSynchronize(st);  // the copy must not outlive us
        ok = false;
      }
      std::lock_guard<std::mutex> g(mu_);
      if (ok) {
        issued_.push_back({i, slot});
        cv_issued_.notify_one();
      } else {
        free_.push_back(slot);
        break;
      }
    }
    std::lock_guard<std::mutex> g(mu_);
    copier_done_ = true;
    cv_issued_.notify_all();
  }

  // Takes completed slots in issue order.  After a failure it keeps
  // draining (waits for each in-flight copy, frees the slot) and writes
  // nothing.
  void ring_writer(int device) {
    (void)hipSetDevice(device);
    while (true) {
      Issued it;
      {
        std::unique_lock<std::mutex> g(mu_);
        cv_issued_.wait(g, [&] { return !issued_.empty() || copier_done_; });
        if (issued_.empty()) return;
        it = issued_.front();
        issued_.pop_front();
      }
      // the event was created with hipEventBlockingSync: this sleeps
      const int64_t t0 = now_ns();
      bool ok = hip(hipEventSynchronize(events_[it.slot]),
                    "hipEventSynchronize");
      const int64_t t1 = now_ns();
      if (ok && !failed())
        write_task(tasks[it.task], (const char*)opt_.ring +
                                       (size_t)it.slot * opt_.chunk_bytes);
      ns_event_wait_ += t1 - t0;
      ns_write_ += now_ns() - t1;
      std::lock_guard<std::mutex> g(mu_);
      free_.push_back(it.slot);
      cv_free_.notify_one();
    }
  }

  // HS_TIMING figures: where the copier and the writers spent their time
  void report(int64_t wall_ns, int nthreads) const {
    std::fprintf(stderr,
                 "[hs-timing] bucket writer: %zu chunks, wall %.3fs, copier "
                 "waited for a free slot %.3fs; %d writers summed: copy "
                 "wait %.3fs, open+pwrite+close %.3fs\n",
                 tasks.size(), wall_ns * 1e-9, ns_slot_wait_.load() * 1e-9,
                 nthreads, ns_event_wait_.load() * 1e-9,
                 ns_write_.load() * 1e-9);
  }

  void close_all() {
    for (size_t f = 0; f < files_.size(); f++) {
      if (plans_[f].fd >= 0) {
        ::close(plans_[f].fd);
        plans_[f].fd = -1;
      }
    }
  }

 private:
  const std::vector<FileJob>& files_;
  const Options& opt_;
  std::vector<FileResult>& results_;
  std::unique_ptr<FilePlan[]> plans_;

  std::atomic<bool> failed_{false};
  std::mutex err_mu_;
  std::string error_;
  std::atomic<size_t> next_{0};
  std::atomic<int64_t> ns_slot_wait_{0}, ns_event_wait_{0}, ns_write_{0};

  std::mutex mu_;  // free_, issued_, copier_done_
  std::condition_variable cv_free_, cv_issued_;
  std::vector<int> free_;
  std::deque<Issued> issued_;
  bool copier_done_ = false;
  hipEvent_t* events_ = nullptr;

  bool hip(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    fail(std::string(what) + ": " + hipGetErrorString(e));
    return false;
  }

  void fail_io(const char* what, const std::string& path) {
    fail(std::string(what) + " " + path + ": " + std::strerror(errno));
  }

  bool pwrite_all(int fd, const char* p, size_t n, int64_t off,
                  const std::string& path) {
    while (n) {
      ssize_t w = ::pwrite(fd, p, n, (off_t)off);
      if (w < 0) {
        if (errno == EINTR) continue;
        fail_io("pwrite", path);
        return false;
      }
      p += w;
      n -= (size_t)w;
      off += w;
    }
    return true;
  }

  // The first thread to touch a file opens it and writes its magic, page
  // headers and footer.
  int ensure_open(int f) {
    FilePlan& fp = plans_[f];
    std::lock_guard<std::mutex> g(fp.open_mu);
    if (!fp.open_tried) {
      fp.open_tried = true;
      const std::string& path = files_[f].path;
      int fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC,
                      0666);
      if (fd < 0) {
        fail_io("open", path);
        return -1;
      }
      fp.fd = fd;
      for (const auto& pc : fp.pieces)
        if (!pwrite_all(fd, pc.second.data(), pc.second.size(), pc.first,
                        path))
          break;
    }
    return failed() ? -1 : fp.fd;
  }

  void write_task(const Task& t, const char* src) {
    int fd = ensure_open(t.file);
    if (fd < 0) return;
    const std::string& path = files_[t.file].path;
    if (!pwrite_all(fd, src, t.nbytes, t.file_off, path)) return;
    FilePlan& fp = plans_[t.file];
    if (fp.remaining.fetch_sub(1, std::memory_order_acq_rel) != 1) return;
    // last chunk of the file: record (size, mtime) and close
    struct stat st;
    if (::fstat(fd, &st) != 0) {
      fail_io("fstat", path);
      return;
    }
    results_[t.file].size = (int64_t)st.st_size;
    results_[t.file].mtime_ns =
        (int64_t)st.st_mtim.tv_sec * 1000000000LL + st.st_mtim.tv_nsec;
    fp.fd = -1;
    if (::close(fd) != 0) fail_io("close", path);
  }
};

}  // namespace

std::string page_header_bytes(int64_t num_values, int64_t nbytes) {
  TWriter w;
  w.struct_begin();
  w.field_i32(1, 0);  // DATA_PAGE
  w.field_i32(2, nbytes);
  w.field_i32(3, nbytes);
  w.field_struct_begin(5);  // DataPageHeader
  w.field_i32(1, num_values);
  w.field_i32(2, 0);  // PLAIN
  w.field_i32(3, 0);  // definition_level_encoding
  w.field_i32(4, 0);  // repetition_level_encoding
  w.struct_end();
  w.struct_end();
  return std::move(w.buf);
}

std::vector<FileResult> write_bucket_files(
    const std::vector<Column>& cols, const std::vector<FileJob>& files,
    const std::vector<std::pair<std::string, std::string>>& stats,
    const Options& opt) {
  const size_t ncols = cols.size(), nfiles = files.size();
  if (stats.size() != nfiles * ncols)
    throw std::invalid_argument("write_bucket_files: stats size mismatch");
  if (opt.chunk_bytes == 0 || opt.writer_threads < 1 ||
      opt.writer_threads > 15)
    throw std::invalid_argument(
        "write_bucket_files: chunk_bytes > 0 and 1 <= writer_threads <= 15");
  int nslots = 0;
  if (opt.device_source) {
    nslots = (int)std::min<size_t>(opt.ring_bytes / opt.chunk_bytes, 4096);
    if (opt.ring == nullptr || nslots < 1)
      throw std::invalid_argument(
          "write_bucket_files: the ring holds no chunk");
  }
  std::vector<FileResult> results(nfiles);
  if (nfiles == 0 || ncols == 0) return results;

  Run run(files, opt, results);
  const std::string magic("PAR1", 4);
  std::vector<std::vector<Task>> file_tasks(nfiles);
  for (size_t f = 0; f < nfiles; f++) {
    const FileJob& job = files[f];
    if (job.row_lo < 0 || job.row_hi <= job.row_lo)
      throw std::invalid_argument("write_bucket_files: empty row range");
    const int64_t rows = job.row_hi - job.row_lo;
    FilePlan& fp = run.plans()[f];
    FileResult& res = results[f];
    fp.pieces.emplace_back(0, magic);
    std::vector<ColMeta> meta(ncols);
    int64_t off = 4;
    int64_t chunks = 0;
    for (size_t c = 0; c < ncols; c++) {
      const int64_t nbytes = rows * cols[c].elem_size;
      std::string header = page_header_bytes(rows, nbytes);
      meta[c] = {off, (int64_t)header.size() + nbytes};
      const int64_t start = off + (int64_t)header.size();
      res.payload_start.push_back(start);
      res.payload_end.push_back(start + nbytes);
      fp.pieces.emplace_back(off, std::move(header));
      const char* src = (const char*)cols[c].base +
                        job.row_lo * (int64_t)cols[c].elem_size;
      for (int64_t done = 0; done < nbytes;) {
        size_t n = (size_t)std::min<int64_t>(nbytes - done,
                                             (int64_t)opt.chunk_bytes);
        file_tasks[f].push_back({(int)f, start + done, src + done, n});
        done += (int64_t)n;
        chunks++;
      }
      off = start + nbytes;
    }
    std::string tail = footer_bytes(cols, meta, rows, &stats[f * ncols]);
    const uint32_t flen = (uint32_t)tail.size();
    char le[4] = {(char)(flen & 0xFF), (char)((flen >> 8) & 0xFF),
                  (char)((flen >> 16) & 0xFF), (char)((flen >> 24) & 0xFF)};
    tail.append(le, 4);
    tail += magic;
    fp.pieces.emplace_back(off, std::move(tail));
    fp.remaining.store(chunks);
  }
  // Issue order: round-robin over groups of kFileGroup files, so that the
  // chunks the writers hold at one time belong to different files.  Writes
  // to one file serialise on its inode lock; in file order the 15 writers
  // would share two or three files.
  for (size_t g = 0; g < nfiles; g += kFileGroup) {
    const size_t g_end = std::min(nfiles, g + kFileGroup);
    for (size_t j = 0;; j++) {
      bool any = false;
      for (size_t f = g; f < g_end; f++) {
        if (j < file_tasks[f].size()) {
          run.tasks.push_back(file_tasks[f][j]);
          any = true;
        }
      }
      if (!any) break;
    }
  }
  file_tasks.clear();

  const int nthreads =
      (int)std::min<size_t>((size_t)opt.writer_threads, run.tasks.size());
  std::vector<std::thread> threads;
  std::vector<hipEvent_t> events;
  const int64_t t_start = now_ns();
  if (opt.device_source) {
    int device = 0;
    hipError_t e = hipGetDevice(&device);
    for (int s = 0; s < nslots && e == hipSuccess; s++) {
      hipEvent_t ev = nullptr;
      e = hipEventCreateWithFlags(
          &ev, hipEventBlockingSync | hipEventDisableTiming);
      if (e == hipSuccess) events.push_back(ev);
    }
    if (e != hipSuccess) {
      run.fail(std::string("hipEventCreate: ") + hipGetErrorString(e));
    } else {
      run.init_ring(nslots, events.data());
      try {
        for (int t = 0; t < nthreads; t++)
          threads.emplace_back([&run, device] { run.ring_writer(device); });
      } catch (const std::exception& ex) {
        run.fail(std::string("thread start: ") + ex.what());
      }
      run.copier();
    }
  } else {
    try {
      for (int t = 0; t < nthreads; t++)
        threads.emplace_back([&run] { run.host_writer(); });
    } catch (const std::exception& ex) {
      run.fail(std::string("thread start: ") + ex.what());
    }
  }
  for (std::thread& t : threads) t.join();
  for (hipEvent_t ev : events) (void)hipEventDestroy(ev);
  run.close_all();
  if (opt.timing) run.report(now_ns() - t_start, nthreads);
  if (run.failed())
    throw std::runtime_error("write_bucket_files: " + run.error());
  return results;
}

}  // namespace hsw
