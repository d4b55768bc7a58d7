// tu_flowinv.hip — nlk_dev_flow_invert of include/nlk_hip.h (kernel: k_flowinv.h)
#include "k_flowinv.h"
#include "nlk_internal.h"

extern "C" int nlk_dev_flow_invert(nlk_ctx* c, float* inv, const float* flow, int w, int h, int iters) {
  const char* who = "nlk_dev_flow_invert";
  if (!c || !inv || !flow) return fail(c, NLK_EINVAL, "%s: NULL argument", who);
  if (inv == flow) return fail(c, NLK_EINVAL, "%s: the result cannot replace the flow (every step reads the flow)", who);
  if (w < 1 || h < 1) return fail(c, NLK_EINVAL, "%s: size %d x %d", who, w, h);
  if (iters < 0 || iters > 16) return fail(c, NLK_EINVAL, "%s: %d steps are outside 0..16", who, iters);
  const unsigned gx = ((unsigned)w + NLK_FLOWINV_BX - 1) / NLK_FLOWINV_BX, gy = ((unsigned)h + NLK_FLOWINV_BY - 1) / NLK_FLOWINV_BY;
  if (gy > 65535u) return fail(c, NLK_EUNSUP, "%s: %d rows are more than one launch covers", who, h);
  NLK_USE_DEVICE(c);
  hipLaunchKernelGGL(k_flow_invert, dim3(gx, gy), dim3(NLK_FLOWINV_BX, NLK_FLOWINV_BY), 0, c->stream,
                     reinterpret_cast<nlk_flow_f2*>(inv), reinterpret_cast<const nlk_flow_f2*>(flow), w, h, iters);
  HIPCHK(c, hipGetLastError());
  return NLK_OK;
}
