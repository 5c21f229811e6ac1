// Payload writer for the filesystem storage backend.
//
// Plain C++17 + POSIX: no HIP, no pybind, so it builds stand-alone (the
// host sanitizer test compiles it with an ordinary C++ compiler) and
// staging.hip only wraps it in a binding.
//
// Two write policies, chosen per call:
//
//   reuse    - the target is an existing regular file and the payload is at
//              least kReuseMinBytes: open WITHOUT O_TRUNC, pwrite over the
//              old content, then ftruncate down only if the old file was
//              longer. A re-save to the same path then reuses the file's
//              page-cache pages instead of freeing and reallocating every
//              one of them (for a 16 GB checkpoint that is ~4 M pages per
//              save, dirty/writeback state included).
//   truncate - everything else (new file, small payload, reuse=false):
//              O_CREAT|O_TRUNC and the same write loop.
//
// One sequential stream per file either way. The Python fallback in
// storage/fs.py follows the same policy, so what lands on disk does not
// depend on whether the extension is built.

#pragma once

#include <cerrno>
#include <cstddef>
#include <cstdint>
#include <string>

#include <fcntl.h>
#include <sys/stat.h>
#include <sys/types.h>
#include <unistd.h>

namespace tsamd {

// payloads below this always take the truncate path (metadata, checksums
// and other small files: nothing to gain, and their old length is arbitrary)
constexpr size_t kReuseMinBytes = 1u << 20;

struct SinkResult {
  int err = 0;            // 0 on success, else errno of the failed call
  const char* op = "";    // which call failed ("open", "pwrite", ...)
  bool reused = false;    // true when the reuse policy was taken
};

namespace detail {

inline int close_noeintr(int fd) {
  // POSIX leaves the fd state unspecified after EINTR; on Linux it is
  // closed, so never retry
  int r = ::close(fd);
  return (r != 0 && errno != EINTR) ? errno : 0;
}

inline int fsync_dir_of(const std::string& path) {
  std::string dir;
  size_t slash = path.find_last_of('/');
  if (slash == std::string::npos) dir = ".";
  else if (slash == 0) dir = "/";
  else dir = path.substr(0, slash);
  int dfd = ::open(dir.c_str(), O_RDONLY | O_DIRECTORY | O_CLOEXEC);
  if (dfd < 0) return errno;
  int err = 0;
  if (::fsync(dfd) != 0) err = errno;
  int cerr = close_noeintr(dfd);
  return err ? err : cerr;
}

}  // namespace detail

// Write data[0, nbytes) to `path`. Never leaks the fd; never throws.
inline SinkResult file_write(const std::string& path, const void* data,
                             size_t nbytes, bool do_fsync, size_t chunk_bytes,
                             bool reuse) {
  SinkResult res;
  if (chunk_bytes == 0) {
    res.err = EINVAL;
    res.op = "chunk_bytes";
    return res;
  }
  int fd = -1;
  off_t old_size = 0;
  if (reuse && nbytes >= kReuseMinBytes) {
    // O_NOFOLLOW is deliberately absent: a symlinked payload behaves as it
    // does on the truncate path. A file that vanished between a listing
    // and this open simply takes the truncate path below.
    fd = ::open(path.c_str(), O_WRONLY | O_CLOEXEC);
    if (fd >= 0) {
      struct stat st;
      if (::fstat(fd, &st) != 0) {
        res.err = errno;
        res.op = "fstat";
        (void)detail::close_noeintr(fd);
        return res;
      }
      if (S_ISREG(st.st_mode)) {
        old_size = st.st_size;
        res.reused = true;
      } else {
        // FIFO, device, ...: today's sequence, whatever it does there
        (void)detail::close_noeintr(fd);
        fd = -1;
      }
    } else if (errno != ENOENT) {
      res.err = errno;
      res.op = "open";
      return res;
    }
  }
  if (fd < 0) {
    fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
    if (fd < 0) {
      res.err = errno;
      res.op = "open";
      return res;
    }
  }

  const char* p = static_cast<const char*>(data);
  size_t off = 0;
  while (off < nbytes) {
    size_t want = nbytes - off < chunk_bytes ? nbytes - off : chunk_bytes;
    ssize_t n = ::pwrite(fd, p + off, want, static_cast<off_t>(off));
    if (n < 0) {
      if (errno == EINTR) continue;
      res.err = errno;
      res.op = "pwrite";
      break;
    }
    if (n == 0) {
      // a regular file never returns 0 for a nonzero count; don't spin
      res.err = EIO;
      res.op = "pwrite";
      break;
    }
    off += static_cast<size_t>(n);  // short write: go round again
  }
  if (!res.err && res.reused && old_size > static_cast<off_t>(nbytes)) {
    int r;
    do {
      r = ::ftruncate(fd, static_cast<off_t>(nbytes));
    } while (r != 0 && errno == EINTR);
    if (r != 0) {
      res.err = errno;
      res.op = "ftruncate";
    }
  }
  if (!res.err && do_fsync) {
    if (::fsync(fd) != 0) {
      res.err = errno;
      res.op = "fsync";
    } else if (int derr = detail::fsync_dir_of(path)) {
      // the directory entry must be durable too: the metadata commit may
      // never be durable before its payloads
      res.err = derr;
      res.op = "fsync(dir)";
    }
  }
  int cerr = detail::close_noeintr(fd);
  if (!res.err && cerr) {
    res.err = cerr;
    res.op = "close";
  }
  return res;
}

}  // namespace tsamd
