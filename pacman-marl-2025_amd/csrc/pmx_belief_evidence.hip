// pmx_belief_evidence.hip -- the EVIDENCE forms of the two belief update kernels (pmx_belief.h; include/pmx.h, "Belief evidence"),
// in a code object of their own so that pmx_step.hip's kernels stay the instructions they were.
#include <hip/hip_ext.h>

#include "pmx_belief.h"

// pmx_belief_update_evidence (weights == NULL: p's set block alone is read) / pmx_belief_weights_update_evidence.  count > 0 rows;
// ev0 / ev1 as in pmx_launch_belief
extern "C" hipError_t pmx_launch_belief_evidence(const PmxBeliefWeightsParams *p, const PmxBeliefEvidenceParams *e, int weighted, hipStream_t st,
                                                 hipEvent_t ev0, hipEvent_t ev1)
{
    const unsigned blocks = (unsigned)(((long)p->b.count + 3) / 4);
    const BeliefEvidenceArg<true> arg{*e};
    if (weighted) {
        if (ev0) hipExtLaunchKernelGGL((pmx_belief_weights_kernel<false, true>), dim3(blocks), dim3(PMX_BLOCK), 0, st, ev0, ev1, 0, *p, arg);
        else hipLaunchKernelGGL((pmx_belief_weights_kernel<false, true>), dim3(blocks), dim3(PMX_BLOCK), 0, st, *p, arg);
    } else {
        if (ev0) hipExtLaunchKernelGGL((pmx_belief_kernel<false, true>), dim3(blocks), dim3(PMX_BLOCK), 0, st, ev0, ev1, 0, p->b, arg);
        else hipLaunchKernelGGL((pmx_belief_kernel<false, true>), dim3(blocks), dim3(PMX_BLOCK), 0, st, p->b, arg);
    }
    return hipGetLastError();
}

