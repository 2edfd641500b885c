// poselib_amd — address spaces of the pointers a kernel fetches from a device-resident argument table.
//
// A pointer that arrives as a kernel argument is known to the compiler as a global address.  A pointer that a kernel LOADS
// from memory (an entry of a group's GroupArgs table, an LMTask, ...) is not: it could be an LDS or a scratch address, so
// every access through it becomes a flat_* instruction, which counts on vmcnt AND lgkmcnt and is kept in order with the LDS
// traffic around it (s_waitcnt vmcnt(0) lgkmcnt(0) between a load and the ds_write that stages it).  The group kernels share
// their bodies with the single-problem kernels; so that they share the generated code as well, each group kernel passes the
// arguments it fetched through globalised() before it calls the body.  scripts/isa_memory_ops.py counts what is left.
#pragma once
#include "pl_kernels.h"

namespace pl {

// CONTRACT: p is device-visible memory - a device allocation or a pinned host mirror mapped into the device's address
// space - or null.  It is never an LDS (__shared__) or stack address.  Null stays null (both address spaces use 0).
// (The integer round trip is what makes the compiler forget the flat origin: a plain address-space cast of a loaded
// pointer, or __builtin_assume(!__builtin_amdgcn_is_shared(p)), still yields flat instructions.)
template <class T> __device__ __forceinline__ T *as_global(T *p) {
    typedef __attribute__((address_space(1))) T GlobalT;
    return (T *)(GlobalT *)(uintptr_t)p;
}

// One globalised copy per argument struct: a new pointer member has exactly one place to go.
__device__ __forceinline__ PointSet globalised(PointSet p) {
    for (int d = 0; d < 5; ++d)
        p.a[d] = as_global(p.a[d]);
    return p;
}
__device__ __forceinline__ SampleArgs globalised(SampleArgs s) {
    s.delta = as_global(s.delta);
    s.flagbits = as_global(s.flagbits);
    s.positions = as_global(s.positions);
    s.ctl = as_global(s.ctl);
    return s;
}
__device__ __forceinline__ GenerateArgs globalised(GenerateArgs g) {
    g.pts = globalised(g.pts);
    g.positions = as_global(g.positions);
    g.samples = as_global(g.samples);
    g.ctl = as_global(g.ctl);
    g.models = as_global(g.models);
    g.num_models = as_global(g.num_models);
    g.blk_tot = as_global(g.blk_tot);
    g.blk_nan = as_global(g.blk_nan);
    g.nan_bits = as_global(g.nan_bits);
    g.stage = as_global(g.stage);
    return g;
}
__device__ __forceinline__ Shadow16Params globalised(Shadow16Params s) {
    s.out = as_global(s.out);
    s.live = as_global(s.live);
    s.rank = as_global(s.rank);
    s.nan_bits = as_global(s.nan_bits);
    s.points16 = as_global(s.points16);
    return s;
}
__device__ __forceinline__ CompactArgs globalised(CompactArgs c) {
    c.num_models = as_global(c.num_models);
    c.blk_tot = as_global(c.blk_tot);
    c.slots = as_global(c.slots);
    c.offsets = as_global(c.offsets);
    c.models = as_global(c.models);
    c.shadow = as_global(c.shadow);
    c.compact64 = as_global(c.compact64);
    c.ctl = as_global(c.ctl);
    c.s16 = globalised(c.s16);
    c.host_offsets = as_global(c.host_offsets);
    return c;
}
__device__ __forceinline__ ScoreArgs globalised(ScoreArgs a) {
    a.pts = globalised(a.pts);
    a.models = as_global(a.models);
    a.slots = as_global(a.slots);
    a.shadow = as_global(a.shadow);
    a.compact64 = as_global(a.compact64);
    a.shadow16 = as_global(a.shadow16);
    a.points16 = as_global(a.points16);
    a.num_hyp = as_global(a.num_hyp);
    a.part_count = as_global(a.part_count);
    a.part_score = as_global(a.part_score);
    a.tickets = as_global(a.tickets);
    a.prune.st = as_global(a.prune.st);
    a.prune.blk_kept = as_global(a.prune.blk_kept);
    a.prune.sel = as_global(a.prune.sel);
    a.prune.kept = as_global(a.prune.kept);
    a.prune.bnd_count = as_global(a.prune.bnd_count);
    a.prune.bnd_score = as_global(a.prune.bnd_score);
    return a;
}
__device__ __forceinline__ FinalizeArgs globalised(FinalizeArgs f) {
    f.num_hyp = as_global(f.num_hyp);
    f.rank = as_global(f.rank);
    f.part_count = as_global(f.part_count);
    f.part_score = as_global(f.part_score);
    f.count = as_global(f.count);
    f.score = as_global(f.score);
    f.kept = as_global(f.kept);
    return f;
}
__device__ __forceinline__ RecordsArgs globalised(RecordsArgs r) {
    r.f = globalised(r.f);
    r.slots = as_global(r.slots);
    r.models = as_global(r.models);
    r.blk_max = as_global(r.blk_max);
    r.blk_min = as_global(r.blk_min);
    r.rec_meta = as_global(r.rec_meta);
    r.rec_models = as_global(r.rec_models);
    r.ctl = as_global(r.ctl);
    r.host_meta = as_global(r.host_meta);
    r.host_models = as_global(r.host_models);
    return r;
}
__device__ __forceinline__ SeqScoreArgs globalised(SeqScoreArgs a) {
    a.pts = globalised(a.pts);
    a.models = as_global(a.models);
    a.cand = as_global(a.cand);
    a.num = as_global(a.num);
    a.count = as_global(a.count);
    a.score = as_global(a.score);
    a.host_count = as_global(a.host_count);
    a.host_score = as_global(a.host_score);
    a.host_cand = as_global(a.host_cand);
    a.ctl_src = as_global(a.ctl_src);
    a.ctl_host = as_global(a.ctl_host);
    return a;
}
__device__ __forceinline__ MaskArgs globalised(MaskArgs m) {
    m.pts = globalised(m.pts);
    m.model = as_global(m.model);
    m.mask = as_global(m.mask);
    m.host_mask = as_global(m.host_mask);
    m.dst.data = as_global(m.dst.data);
    m.dst.order = as_global(m.dst.order);
    return m;
}
__device__ __forceinline__ SelectArgs globalised(SelectArgs s) {
    s.score_refined = as_global(s.score_refined);
    s.rec_refined = as_global(s.rec_refined);
    s.rec_incumbent = as_global(s.rec_incumbent);
    s.out = as_global(s.out);
    s.count_refined = as_global(s.count_refined);
    s.count_out = as_global(s.count_out);
    s.fetch_src = as_global(s.fetch_src);
    s.fetch_dst = as_global(s.fetch_dst);
    return s;
}
__device__ __forceinline__ PrepareGroupArgs globalised(PrepareGroupArgs p) {
    p.a_raw = as_global(p.a_raw);
    p.b_raw = as_global(p.b_raw);
    p.soa = as_global(p.soa);
    p.absmax_bits = as_global(p.absmax_bits);
    p.stats = as_global(p.stats);
    return p;
}

// The pointer members of an LMTask (the LM kernels keep the task itself in LDS and read its scalars there).  T.pts of the
// result is what the task names in device memory; a kernel that stages the correspondences in LDS when they fit keeps a
// second PointSet that may point either way - those accesses are flat by necessity.
struct LMTaskPointers {
    PointSet pts;
    const uint8_t *mask;
    uint8_t *scratch;
    const double *record_in;
    double *record_out;
    const double *start_record;
    const uint32_t *gate_count;
};
__device__ __forceinline__ LMTaskPointers globalised(const LMTask &T) {
    LMTaskPointers g;
    g.pts = globalised(T.pts);
    g.mask = as_global(T.mask);
    g.scratch = as_global(T.scratch);
    g.record_in = as_global(T.record_in);
    g.record_out = as_global(T.record_out);
    g.start_record = as_global(T.start_record);
    g.gate_count = as_global(T.gate_count);
    return g;
}

} // namespace pl
