// Workspace arithmetic of libmgp_hip: host-only, no HIP include (mgp_common.h includes it; the policy headers and their CPU
// tests use it alone).
#pragma once
#include <stdint.h>
#include <stddef.h>

static inline int64_t mgp_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline size_t mgp_align(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// bump allocator over the caller's workspace
struct MgpArena {
  char* base;
  size_t cap;
  size_t off;
  MgpArena(void* p, size_t bytes) : base(static_cast<char*>(p)), cap(bytes), off(0) {}
  // counting mode: no memory behind it and no limit; take() only advances `off` (the bytes a real arena needs) and returns null
  MgpArena() : base(nullptr), cap(SIZE_MAX), off(0) {}
  template <typename T>
  T* take(size_t count) {
    size_t bytes = mgp_align(count * sizeof(T));
    if (off + bytes > cap) { off = cap + 1; return nullptr; }
    T* r = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += bytes;
    return r;
  }
  bool ok() const { return off <= cap; }
};
