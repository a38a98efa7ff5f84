// Workspace layout of the units that take one caller-allocated void* ws, free of HIP headers: tools/ws_carve_check.cpp walks
// it on the host under ASan + UBSan.
//
// A unit writes its layout once, as a function that takes its parts from a WsCarve in order; the exported dns_*_ws_bytes runs
// that function on a NULL base (every pointer is then NULL and only the end counts) and the launch wrapper on the real one, so
// the size and the pointers cannot drift apart.
#pragma once
#include <stddef.h>
#include <stdint.h>
namespace dns {

inline size_t align256(size_t b) { return (b + 255) & ~size_t(255); }      // workspaces are carved into 256-byte aligned parts
constexpr uint32_t SCAN_THREADS = 1024;  // the one workgroup that scans the carries in a workspace (dev_reduce.hpp's carry_scan)

struct WsCarve {
  char* base;                                                    // NULL: size only
  size_t off = 0;                                                // end of the last part taken
  explicit WsCarve(void* ws) : base((char*)ws) {}
  // The next part, count elements of T: from the previous end rounded up to 256.
  template <class T>
  T* take(uint64_t count) {
    const size_t at = align256(off);
    off = at + (size_t)count * sizeof(T);
    return base ? (T*)(base + at) : nullptr;
  }
  size_t end() const { return off; }                             // the last part's own end
  size_t end256() const { return align256(off); }                // ... rounded up to 256
};

}  // namespace dns
