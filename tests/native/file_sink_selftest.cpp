// Stand-alone check of ops/hip/file_sink.h, meant to be compiled with
// -fsanitize=address,undefined and run directly (see
// tests/test_file_sink_sanitized.py). Usage: file_sink_selftest <empty dir>
// Exit status 0 = every case passed.

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <dirent.h>
#include <sys/stat.h>

#include "file_sink.h"

namespace {

constexpr size_t kMiB = 1u << 20;
constexpr size_t kChunk = 256 * kMiB;
int g_failures = 0;

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failures;                                                      \
    }                                                                    \
  } while (0)

std::vector<unsigned char> pattern(size_t n, unsigned seed) {
  std::vector<unsigned char> v(n);
  for (size_t i = 0; i < n; ++i) {
    v[i] = (unsigned char)((i % 4099) * 7 + seed);
  }
  return v;
}

std::vector<unsigned char> slurp(const std::string& path) {
  std::vector<unsigned char> out;
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) return out;
  unsigned char buf[1 << 16];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) {
    out.insert(out.end(), buf, buf + n);
  }
  std::fclose(f);
  return out;
}

ino_t inode_of(const std::string& path) {
  struct stat st;
  return ::stat(path.c_str(), &st) == 0 ? st.st_ino : 0;
}

int open_fds() {
  int n = 0;
  DIR* d = ::opendir("/proc/self/fd");
  if (!d) return -1;
  while (::readdir(d)) ++n;
  ::closedir(d);
  return n;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s <empty dir>\n", argv[0]);
    return 2;
  }
  const std::string dir = argv[1];
  const std::string p = dir + "/payload";
  const int fds_before = open_fds();

  // fresh
  auto a = pattern(2 * kMiB, 1);
  auto r = tsamd::file_write(p, a.data(), a.size(), false, kChunk, true);
  CHECK(r.err == 0 && !r.reused);
  CHECK(slurp(p) == a);
  const ino_t ino = inode_of(p);

  // shorter, in place, 4 KiB chunks (many pwrites + a 13-byte tail)
  auto b = pattern(kMiB + 13, 2);
  r = tsamd::file_write(p, b.data(), b.size(), false, 4096, true);
  CHECK(r.err == 0 && r.reused);
  CHECK(inode_of(p) == ino);
  CHECK(slurp(p) == b);

  // longer, in place, with fsync of file and directory
  auto c = pattern(3 * kMiB + 1, 3);
  r = tsamd::file_write(p, c.data(), c.size(), true, kChunk, true);
  CHECK(r.err == 0 && r.reused);
  CHECK(slurp(p) == c);

  // reuse=false: truncate path
  r = tsamd::file_write(p, b.data(), b.size(), false, kChunk, false);
  CHECK(r.err == 0 && !r.reused);
  CHECK(slurp(p) == b);

  // tiny payload over a longer file: truncate path, exact size
  auto t = pattern(kMiB - 1, 4);
  r = tsamd::file_write(p, t.data(), t.size(), false, kChunk, true);
  CHECK(r.err == 0 && !r.reused);
  CHECK(slurp(p) == t);

  // empty payload (null data pointer) leaves an empty file
  r = tsamd::file_write(p, nullptr, 0, false, kChunk, true);
  CHECK(r.err == 0 && !r.reused);
  CHECK(slurp(p).empty());

  // error paths: missing directory, directory as target, bad chunk size
  for (size_t n : {size_t(16), 2 * kMiB}) {
    r = tsamd::file_write(dir + "/missing/payload", a.data(), n, false,
                          kChunk, true);
    CHECK(r.err == ENOENT);
    r = tsamd::file_write(dir, a.data(), n, false, kChunk, true);
    CHECK(r.err == EISDIR);
    // opens fine, every write fails: the error path after open
    r = tsamd::file_write("/dev/full", a.data(), n, false, kChunk, true);
    CHECK(r.err == ENOSPC || r.err == ENOENT || r.err == EACCES);
  }
  r = tsamd::file_write(p, a.data(), 16, false, 0, true);
  CHECK(r.err == EINVAL);

  CHECK(open_fds() == fds_before);

  if (g_failures == 0) std::puts("file_sink selftest OK");
  return g_failures == 0 ? 0 : 1;
}
