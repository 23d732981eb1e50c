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
  char* h_stage = nullptr;  // pinned staging of inputs and outputs
  size_t h_bytes = 0;
  char* d_in = nullptr;     // device copy of the staged inputs
  size_t d_in_bytes = 0;
  double* d_work = nullptr; // partials / outputs
  size_t d_work_bytes = 0;
};

// kde.hip
int kde_state(gpmi_ctx* c, KdeState*& st);  // the handle's state, created (with its stream) on first use
int kde_grow_pinned(gpmi_ctx* c, KdeState* st, size_t bytes);
int kde_grow_device(gpmi_ctx* c, void** ptr, size_t* have, size_t bytes);
inline size_t kde_align256(size_t b) { return (b + 255) & ~(size_t)255; }
// kde2d.hip
void kde2d_free(gpmi_kde2d* k);
// unimodal.hip
void unimodal_free(gpmi_unimodal* k);
