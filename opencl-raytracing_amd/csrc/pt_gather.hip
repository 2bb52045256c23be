// pt_gather.hip — the kernels of rt_render_hemispheres (pt_samples_q_hemi, pt_render_hemi), a translation unit of their own
// per arithmetic policy: compiled with pt_kernels.hip's flags, once per policy, and linked beside it.  They are made of the
// device code the other sample kernels are made of — the queue, its sums, the fixed-lane body — which is the text of
// pt_kernels.hip: it is read here once more with PT_GATHER_UNIT set, which leaves out its launchers and the kernels that are
// no templates and instantiates the gather kernels alone (pt::GatherKernels, pt_kernels.hpp).  So the policy's own code
// object holds the kernels it held, and tools/isa_stats.py --unit pt_gather lists these.
#define PT_GATHER_UNIT 1
#include "pt_kernels.hip"
