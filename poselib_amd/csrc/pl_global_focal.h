// poselib_amd — pl_global.h's globalised copies for the argument structs of the focal-length estimators (focal.hip, sfocal.hip)
#pragma once
#include "pl_global.h"
#include "pl_sfocal.h"

namespace pl {

__device__ __forceinline__ FocalGenArgs globalised(FocalGenArgs g) {
    for (int d = 0; d < 5; ++d)
        g.a[d] = as_global(g.a[d]);
    g.positions = as_global(g.positions);
    g.samples = as_global(g.samples);
    g.models = as_global(g.models);
    g.num_models = as_global(g.num_models);
    g.stage = as_global(g.stage);
    g.explicit_in = as_global(g.explicit_in);
    g.host_models = as_global(g.host_models);
    g.host_num_models = as_global(g.host_num_models);
    return g;
}
__device__ __forceinline__ FocalScoreArgs globalised(FocalScoreArgs a) {
    for (int d = 0; d < 5; ++d)
        a.a[d] = as_global(a.a[d]);
    a.models = as_global(a.models);
    a.num_models = as_global(a.num_models);
    a.lm_tasks = as_global(a.lm_tasks);
    a.counts = as_global(a.counts);
    a.sums = as_global(a.sums);
    return a;
}
__device__ __forceinline__ FocalMaskArgs globalised(FocalMaskArgs a) {
    for (int d = 0; d < 5; ++d)
        a.a[d] = as_global(a.a[d]);
    a.mask = as_global(a.mask);
    a.host_mask = as_global(a.host_mask);
    a.dst = as_global(a.dst);
    a.dst_order = as_global(a.dst_order);
    return a;
}
__device__ __forceinline__ SFocalGenArgs globalised(SFocalGenArgs g) {
    for (int d = 0; d < 4; ++d)
        g.a[d] = as_global(g.a[d]);
    g.positions = as_global(g.positions);
    g.samples = as_global(g.samples);
    g.models = as_global(g.models);
    g.num_models = as_global(g.num_models);
    g.host_models = as_global(g.host_models);
    g.host_num_models = as_global(g.host_num_models);
    g.stage = as_global(g.stage);
    g.explicit_in = as_global(g.explicit_in);
    return g;
}
__device__ __forceinline__ SFocalScoreArgs globalised(SFocalScoreArgs a) {
    for (int d = 0; d < 4; ++d)
        a.a[d] = as_global(a.a[d]);
    a.models = as_global(a.models);
    a.num_models = as_global(a.num_models);
    a.lm_tasks = as_global(a.lm_tasks);
    a.counts = as_global(a.counts);
    a.scores = as_global(a.scores);
    return a;
}
// the pointer members of an SFocalLMTask (k_sfocal_lm keeps the task itself in LDS)
struct SFocalLMTaskPointers {
    const double *a[4];
    const uint8_t *mask;
    uint8_t *scratch;
};
__device__ __forceinline__ SFocalLMTaskPointers globalised(const SFocalLMTask &T) {
    SFocalLMTaskPointers g;
    for (int d = 0; d < 4; ++d)
        g.a[d] = as_global(T.a[d]);
    g.mask = as_global(T.mask);
    g.scratch = as_global(T.scratch);
    return g;
}

} // namespace pl
