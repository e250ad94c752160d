// Native replay of a planned kernel program: one C call enqueues every launch of the forward or
// backward plan on its HIP streams, with the cross-stream dependencies expressed as events.
// (The Python planner builds the op list once; per step the host does O(1) Python work.)
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "common.cuh"

namespace {
struct Program {
    std::vector<stl_op> ops;
    std::vector<hipEvent_t> ev;  // one per op with record != 0
    std::vector<int> ev_of;      // op index -> event index or -1
    hipEvent_t fork = nullptr;
    std::vector<hipEvent_t> join;
    int nstreams = 1;
};
}  // namespace

// Flags of the program's cross-stream events.  A default HIP event performs a SYSTEM-scope fence (cache write-back and
// invalidation, "and the performance impact of those actions on the execution of following work", hip_runtime_api.h) when it is
// recorded; producers and consumers of a program's events are kernels on the SAME device, for which device scope orders the data
// (the host reads results only behind a stream / device synchronisation, which fences on its own).  Round 3, one call, two rounds:
// 14.69-14.71 ms per step with the default flags, 14.52-14.57 with hipEventDisableSystemFence, 14.66-14.71 with
// hipEventReleaseToDevice; stream memory operations (hipStreamWriteValue32 / WaitValue32) instead of events: 15.45 (removed).
// Round 5: STLPOSE_EVENT_FENCE=system (read when a program is created) restores the default, fencing events -- the A/B arm of
// tests/test_visibility_gpu.py, which hands 64 MB buffers from stream to stream through a program 2000 times and replays the
// benchmarked train step 300 times under both settings; no stale read under either (the round-4 wrong result was
// an undersized statistics arena, engine.bn_weight_keys, not visibility: every kernel dispatch carries its own agent-scope
// acquire and release, the event's fence only adds the system scope).
static unsigned event_flags() {
    const char* e = getenv("STLPOSE_EVENT_FENCE");
    if (e && strcmp(e, "system") == 0) return hipEventDisableTiming;
    return hipEventDisableTiming | hipEventDisableSystemFence;
}

// one op of a program on stream `st`
static int run_op(const stl_op& o, void* st, int i) {
    int rc;
        switch (o.kind) {
            case STL_OP_CONV: rc = stl_conv_forward(static_cast<const stl_conv*>(o.desc), st); break;
            case STL_OP_WGRAD: rc = stl_conv_wgrad(static_cast<const stl_wgrad*>(o.desc), st); break;
            case STL_OP_WGRAD_GROUP: rc = stl_conv_wgrad_group(static_cast<const stl_wgrad_group*>(o.desc), st); break;
            case STL_OP_FUSE: rc = stl_fuse_forward(static_cast<const stl_fuse*>(o.desc), st); break;
            case STL_OP_FUSE_BWD: rc = stl_fuse_backward(static_cast<const stl_fuse_bwd*>(o.desc), st); break;
            case STL_OP_UP_BWD: rc = stl_upsample_backward(static_cast<const stl_upbwd*>(o.desc), st); break;
            case STL_OP_PATCH: {
                const stl_patch* a = static_cast<const stl_patch*>(o.desc);
                rc = stl_patch3x3(a->dtype, a->img, a->out, a->B, a->H, a->W, a->stride, a->mean3, a->std3, st);
                break;
            }
            case STL_OP_PATCH_BWD: {
                const stl_patch_bwd* a = static_cast<const stl_patch_bwd*>(o.desc);
                rc = stl_patch3x3_backward(a->dtype, a->dpatch, a->dimg, a->B, a->H, a->W, a->stride, a->std3, st);
                break;
            }
            case STL_OP_HEAD: {
                const stl_head* a = static_cast<const stl_head*>(o.desc);
                rc = stl_head_forward(a->dtype, a->x, a->w, a->bias, a->out, a->B, a->H, a->W, a->Ci, a->J, st);
                break;
            }
            case STL_OP_HEAD_BWD: {
                const stl_head_bwd* a = static_cast<const stl_head_bwd*>(o.desc);
                rc = stl_head_backward(a->dtype, a->x, a->w, a->dout, a->dx, a->partial, a->nblk, a->B, a->H, a->W, a->Ci, a->J, st);
                break;
            }
            case STL_OP_REDUCE_RANGE: rc = stl_reduce_slabs_range(static_cast<const stl_reduce_range*>(o.desc), st); break;
            case STL_OP_BN_GRADS_RANGE: {
                const stl_bn_range* a = static_cast<const stl_bn_range*>(o.desc);
                rc = stl_bn_param_grads(a->rstats, a->grads, a->tab, a->n, st);
                break;
            }
            default: return stl_set_error("program_run: op %d has unknown kind %d", i, o.kind);
        }
    return rc;
}

extern "C" int stl_program_create(const stl_op* ops, int n, int nstreams, void** out) {
    STL_CHECK(ops && out && n >= 0 && nstreams >= 1 && nstreams <= 16, "program_create: bad arguments");
    Program* p = new Program();
    p->ops.assign(ops, ops + n);
    p->nstreams = nstreams;
    p->ev_of.assign(n, -1);
    for (int i = 0; i < n; ++i) {
        const stl_op& o = ops[i];
        if (o.stream < 0 || o.stream >= nstreams || o.nwait < 0 || o.nwait > 8 || !o.desc) {
            delete p;
            return stl_set_error("program_create: op %d malformed (stream %d, nwait %d)", i, o.stream, o.nwait);
        }
        for (int w = 0; w < o.nwait; ++w)
            if (o.wait[w] < 0 || o.wait[w] >= i || !ops[o.wait[w]].record) {
                delete p;
                return stl_set_error("program_create: op %d waits on op %d which does not record an earlier event", i, o.wait[w]);
            }
        if (o.record) {
            hipEvent_t e;
            // gradient-bucket ends are picked up from OUTSIDE the program (stl_program_wait_op: the communication stream of a
            // data-parallel run, whose collective may hand the bucket to other devices): those few keep the system-scope fence
            if (hipEventCreateWithFlags(&e, o.kind == STL_OP_BN_GRADS_RANGE ? (unsigned)hipEventDisableTiming : event_flags()) != hipSuccess) {
                delete p;
                return stl_set_error("program_create: hipEventCreate failed");
            }
            p->ev_of[i] = (int)p->ev.size();
            p->ev.push_back(e);
        }
    }
    (void)hipEventCreateWithFlags(&p->fork, event_flags());
    p->join.resize(nstreams);
    for (int s = 0; s < nstreams; ++s) (void)hipEventCreateWithFlags(&p->join[s], event_flags());
    *out = p;
    return 0;
}

extern "C" int stl_program_destroy(void* h) {
    Program* p = static_cast<Program*>(h);
    if (!p) return 0;
    for (hipEvent_t e : p->ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : p->join) (void)hipEventDestroy(e);
    if (p->fork) (void)hipEventDestroy(p->fork);
    delete p;
    return 0;
}

extern "C" int stl_program_wait_op(void* h, int op, void* stream) {
    Program* p = static_cast<Program*>(h);
    STL_CHECK(p && op >= 0 && op < (int)p->ops.size() && p->ev_of[op] >= 0, "program_wait_op: op %d does not record an event", op);
    STL_CHECK(hipStreamWaitEvent((hipStream_t)stream, p->ev[p->ev_of[op]], 0) == hipSuccess, "program_wait_op: wait failed");
    return 0;
}

// ops [first, last) of the program; the first range forks the side streams off the main stream, the last one joins them.
// Splitting a run lets the host put other work between two ranges IN ISSUE ORDER: hardware queues are in-order and the
// communication stream of a data-parallel run shares one with a compute stream (four hardware queues), so a gradient bucket's
// all-reduce must be ENQUEUED right behind the bucket's last op -- issued after the whole backward program it would sit behind
// everything that queue still has to run (measured with a stand-in kernel, profiles/r04_dp_overlap*.txt: bucket 0 final at
// 6.3 ms, its communication-stream kernel started at 13.9 ms).
extern "C" int stl_program_run_range(void* h, void* const* streams, int first, int last) {
    Program* p = static_cast<Program*>(h);
    STL_CHECK(p && streams, "program_run: null program");
    const int n = (int)p->ops.size();
    STL_CHECK(first >= 0 && first <= last && last <= n, "program_run_range: bad range [%d, %d) of %d ops", first, last, n);
    hipStream_t main = (hipStream_t)streams[0];
    if (first == 0 && p->nstreams > 1) {
        STL_CHECK(hipEventRecord(p->fork, main) == hipSuccess, "program_run: fork record failed");
        for (int s = 1; s < p->nstreams; ++s)
            STL_CHECK(hipStreamWaitEvent((hipStream_t)streams[s], p->fork, 0) == hipSuccess, "program_run: fork wait failed");
    }
    for (int i = first; i < last; ++i) {
        const stl_op& o = p->ops[i];
        void* st = streams[o.stream];
        for (int w = 0; w < o.nwait; ++w)
            STL_CHECK(hipStreamWaitEvent((hipStream_t)st, p->ev[p->ev_of[o.wait[w]]], 0) == hipSuccess, "program_run: wait failed");
        int rc = run_op(o, st, i);
        if (rc != 0) return rc;
        if (o.record) STL_CHECK(hipEventRecord(p->ev[p->ev_of[i]], (hipStream_t)st) == hipSuccess, "program_run: record failed");
    }
    if (last == n) {
        for (int s = 1; s < p->nstreams; ++s) {
            STL_CHECK(hipEventRecord(p->join[s], (hipStream_t)streams[s]) == hipSuccess, "program_run: join record failed");
            STL_CHECK(hipStreamWaitEvent(main, p->join[s], 0) == hipSuccess, "program_run: join wait failed");
        }
    }
    return 0;
}

extern "C" int stl_program_run(void* h, void* const* streams) {
    Program* p = static_cast<Program*>(h);
    STL_CHECK(p && streams, "program_run: null program");
    return stl_program_run_range(h, streams, 0, (int)p->ops.size());
}

