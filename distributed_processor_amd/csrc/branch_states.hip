// branch_states.hip -- branch_kernel (branch_kernel.h) with the prepared
// states supplied by the caller (FEAT_STATES: dpemu_run_states, lane.h
// meas_bit_given), every program feature combination.  Pulse-only and
// branch-free register programs run here too (the combinations without
// FEAT_FPROC / FEAT_LUT / FEAT_SYNC).
#include "branch_kernel.h"

namespace dpemu {

hipError_t launch_branch_states(const KParams &p, int feat, uint32_t blocks, hipStream_t stream)
{
    switch (feat & (FEAT_FPROC | FEAT_LUT | FEAT_SYNC | FEAT_REGS | FEAT_PROG_LDS | FEAT_STATES)) {
#define CASE(F) case F: return launch_branch_f<F>(p, blocks, stream);
#define CASES(L) CASE(L) CASE(L | FEAT_FPROC) CASE(L | FEAT_SYNC) CASE(L | FEAT_FPROC | FEAT_SYNC) \
                 CASE(L | FEAT_LUT) CASE(L | FEAT_LUT | FEAT_SYNC)
    CASES(FEAT_STATES) CASES(FEAT_STATES | FEAT_REGS) CASES(FEAT_STATES | FEAT_PROG_LDS)
    CASES(FEAT_STATES | FEAT_REGS | FEAT_PROG_LDS)
#undef CASES
#undef CASE
    }
    return hipErrorInvalidValue;
}

}  // namespace dpemu
