// Per-handle state shared by the density entry points (kde.hip: gpmi_kde_*, kde2d.hip: gpmi_kde2d_*, unimodal.hip:
// gpmi_unimodal_*): one stream and
// workspaces for every density object of the handle (calls on one handle are serialised), and the live objects, which
// gpmi_destroy releases.  Internal.
#pragma once
#include <vector>

#include "api_internal.h"

struct gpmi_kde;
struct gpmi_kde2d;
struct gpmi_unimodal;

struct KdeState {
  hipStream_t stream = nullptr;
  std::vector<gpmi_kde*> live;
  std::vector<gpmi_kde2d*> live2d;
  std::vector<gpmi_unimodal*> live_uni;
  PinBuf<char> h_stage;  // pinned staging of inputs and outputs
  DevBuf<char> d_in;     // device copy of the staged inputs
  DevBuf<char> d_work;   // partials / outputs
  double* work() const { return reinterpret_cast<double*>(d_work.get()); }
  // at least `bytes` of each, 64 KiB to begin with
  static int64_t floor64k(size_t bytes) { return (int64_t)std::max(bytes, (size_t)1 << 16); }
  int reserve_pinned(gpmi_ctx* c, size_t bytes) { return h_stage.reserve(c, floor64k(bytes), hipHostMallocPortable); }
  int reserve_in(gpmi_ctx* c, size_t bytes) { return d_in.reserve(c, floor64k(bytes)); }
  int reserve_work(gpmi_ctx* c, size_t bytes) { return d_work.reserve(c, floor64k(bytes)); }
};

// kde.hip
int kde_state(gpmi_ctx* c, KdeState*& st);  // the handle's state, created (with its stream) on first use
// buf <- the n elements at `host`, for a new object of the entry point `who` (which the error text names)
template <class T>
int kde_upload(gpmi_ctx* c, DevBuf<T>& buf, const T* host, int64_t n, const char* who) {
  int rc = buf.alloc(c, n);
  if (!rc) {
    const hipError_t e = hipMemcpy(buf, host, sizeof(T) * (size_t)n, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      c->err = hipGetErrorString(e);
      rc = GPMI_ERR_HIP;
    }
  }
  if (rc) c->err = std::string(who) + ": " + c->err;
  return rc;
}
inline size_t kde_align256(size_t b) { return (b + 255) & ~(size_t)255; }
// kde2d.hip, unimodal.hip: delete the object (its type is complete only there)
void kde2d_free(gpmi_kde2d* k);
void unimodal_free(gpmi_unimodal* k);
