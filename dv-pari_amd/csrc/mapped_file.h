// A whole file mapped read-only, and the little-endian reads of the on-disk formats (host only, plain C++: cache.cpp and tree_io.cpp
// also build without the HIP compiler).  Used by cache.cpp, tree_io.cpp and setup.hip.
#pragma once
#include <fcntl.h>
#include <stdint.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "../../include/dvpari.h"

namespace dvp {

struct MappedFile {
  const uint8_t* p = nullptr;
  size_t len = 0;
  int fd = -1;
  MappedFile() = default;
  MappedFile(const MappedFile&) = delete;
  MappedFile& operator=(const MappedFile&) = delete;
  ~MappedFile() {
    if (p) munmap((void*)p, len);
    if (fd >= 0) close(fd);
  }
  // DVP_EIO when the file cannot be opened or mapped.  An EMPTY file opens, with len == 0 and p == nullptr: the formats with a length
  // prefix refuse it where they look for the prefix, and a caller without one says so itself
  int open_ro(const char* path) {
    fd = ::open(path, O_RDONLY);
    if (fd < 0) return DVP_EIO;
    struct stat st;
    if (fstat(fd, &st) != 0) return DVP_EIO;
    if (st.st_size == 0) return DVP_OK;
    void* q = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (q == MAP_FAILED) return DVP_EIO;
    p = (const uint8_t*)q;
    len = (size_t)st.st_size;
    return DVP_OK;
  }
};

inline uint64_t rd64le(const uint8_t* p) {
  uint64_t v;
  memcpy(&v, p, 8);
  return v;
}
inline uint32_t rd32le(const uint8_t* p) {
  uint32_t v;
  memcpy(&v, p, 4);
  return v;
}

}  // namespace dvp
