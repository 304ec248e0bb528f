// side_lib.h -- what every library beside libvtx.so (aug, randaug, views, mix, stem, ragged, dropout, yuv, yuv10) defines for itself.
//
// common.h declares vtx::set_error and vtx::check_launch; api.hip holds libvtx.so's definitions.  A side library shares
// nothing with libvtx.so, so it carries its own: VTX_SIDE_LIB(name), written once at file scope of the library's one
// source file, expands to the thread-local message buffer, the two helpers, vtx_<name>_version and
// vtx_<name>_last_error_string.  The link is -Bsymbolic: each library calls its own definitions, whatever else the
// process has loaded.
#pragma once
#include <stdarg.h>
#include "common.h"

#define VTX_SIDE_LIB(name)                                                              \
  namespace vtx {                                                                       \
  static thread_local char g_##name##_err[512] = "";                                    \
  void set_error(const char* fmt, ...) {                                                \
    va_list ap;                                                                         \
    va_start(ap, fmt);                                                                  \
    vsnprintf(g_##name##_err, sizeof(g_##name##_err), fmt, ap);                         \
    va_end(ap);                                                                         \
  }                                                                                     \
  int check_launch(const char* what) {                                                  \
    hipError_t e = hipGetLastError();                                                   \
    if (e != hipSuccess) {                                                              \
      set_error("%s: launch failed: %s", what, hipGetErrorString(e));                   \
      return VTX_ELAUNCH;                                                               \
    }                                                                                   \
    return VTX_OK;                                                                      \
  }                                                                                     \
  }                                                                                     \
  extern "C" int vtx_##name##_version(void) { return 100; } /* 0.1.0 */                 \
  extern "C" const char* vtx_##name##_last_error_string(void) { return vtx::g_##name##_err; }

namespace vtx {

// workgroups of 256 threads for `work` items of a grid-stride kernel, at most `cap` (the kernel walks the rest)
static inline int grid_for(long work, int cap) {
  const long g = (work + 255) / 256;
  return (int)(g > cap ? cap : (g < 1 ? 1 : g));
}

}  // namespace vtx
