// Host side of libnlc_hip.so, snapshot selection: nlc_train_keep_best (kernels_train_select.hip), the reference's
// save-on-improvement (train_utils.py:439-448) for the M members of a trainer in two launches.  It reads no model from the
// ctx: the NL and RNN trainers share it.
#include "nlc_host.h"
#include "nlc_train_select.h"

using namespace nlc;
using namespace nlc::host;
using namespace nlc::train;

// train_utils.py:439-448 (save on improvement), :491 (best_val_loss)
extern "C" int nlc_train_keep_best(nlc_ctx* c, int M, int64_t P, const double* loss, const double* params, double* best_loss,
                                   double* best_params, int64_t* best_tag, int64_t tag, int32_t* improved) {
  if (!c) return NLC_ERR_BAD_ARG;
  NLC_GUARD_BEGIN
  // all on the host, before any launch
  if (!loss || !params || !best_loss || !best_params || !best_tag) return fail(c, NLC_ERR_BAD_ARG, "NULL device pointer");
  if (params == best_params)
    return fail(c, NLC_ERR_BAD_ARG, "keep_best: params_dev and best_params_dev must be different buffers");
  if ((((uintptr_t)params | (uintptr_t)best_params) & 7) != 0)
    return fail(c, NLC_ERR_BAD_ARG, "keep_best: parameter buffers must be 8-byte aligned");
  if (M < 1) return fail(c, NLC_ERR_BAD_SHAPE, "keep_best: a group needs M >= 1 members");
  if (P < 1) return fail(c, NLC_ERR_BAD_SHAPE, "keep_best: P must be >= 1");
  if (M > kSelectMaxGroup) return fail(c, NLC_ERR_UNSUPPORTED, "keep_best: at most 65535 members in a group");
  if (select_chunks(P) > kSelectMaxChunks) return fail(c, NLC_ERR_UNSUPPORTED, "keep_best: P is past the grid's x limit");
  NLC_HIP(c, hipSetDevice(c->device));
  const KeepBestArgs a{loss, params, best_loss, best_params, best_tag, improved, P, tag, M};
  {
    ProfScope ps(c, "train_keep_best_kernel");
    NLC_HIP(c, launch_train_keep_best(a, c->stream));
  }
  ProfScope ps(c, "train_commit_best_kernel");
  NLC_HIP(c, launch_train_commit_best(a, c->stream));
  return NLC_OK;
  NLC_GUARD_END(c)
}
