// poll.hpp -- the polled device loop the iterative pressure solvers share
// (poisson_solve.hpp: CG, BiCGSTAB; relax_solve.hip; transform_solve.hpp reads
// a final state through it). Host templates only.
#pragma once

#include "ctx.hpp"

#include <type_traits>

// ---------------------------------------------------------------------------
// The polled device loop. A solver keeps its state (S: CgState, BcgState,
// RxState) on the device, where the kernels decide when it is done; the host
// launches steps in chunks and polls a pinned copy of the state once per
// chunk, one chunk behind (double-buffered), so the stream never drains
// while it waits. Steps launched after the decision return at once. On
// Z-slabs every rank sees the same all-reduced state and leaves at the same
// chunk.
// ---------------------------------------------------------------------------
template <class S>
static S poll_slot(const hip_proj_ctx* c, int slot) {
    static_assert(sizeof(S) <= sizeof(PollSlot) && std::is_trivially_copyable<S>::value,
                  "the pinned poll slots hold a raw copy of the state");
    S s;
    memcpy(&s, c->h_state[slot].bytes, sizeof(S));
    return s;
}

// step(it) launches one step and advances it (by 1; a k_rb2 sweep by 2, past
// `end` when it comes to that). The chunk starts at 8 steps and doubles up
// to cfg.poll_interval.
template <class S, class Step>
static cfd_status_t poll_loop(hip_proj_ctx* c, const S* dstate, int& it, int end, Step&& step) {
    int chunk = 8, slot = 0, prev = -1;
    const int chunk_max = std::max(1, c->cfg.poll_interval);
    while (it < end) {
        const int chunk_target = it + chunk;
        while (it < end && it < chunk_target) ST_TRY(step(it));
        HIP_TRY(hipMemcpyAsync(c->h_state[slot].bytes, dstate, sizeof(S), hipMemcpyDeviceToHost,
                               c->stream));
        HIP_TRY(hipEventRecord(c->ev_poll[slot], c->stream));
        if (prev >= 0) {
            HIP_TRY(hipEventSynchronize(c->ev_poll[prev]));
            if (poll_slot<S>(c, prev).done) break;
        }
        prev = slot;
        slot ^= 1;
        chunk = std::min(chunk * 2, chunk_max);
    }
    return CFD_SUCCESS;
}

// The state after everything launched so far, read through the third slot.
template <class S>
static cfd_status_t poll_final(hip_proj_ctx* c, const S* dstate, S* out) {
    HIP_TRY(hipMemcpyAsync(c->h_state[2].bytes, dstate, sizeof(S), hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *out = poll_slot<S>(c, 2);
    return CFD_SUCCESS;
}

// The solve's statistics from its final state (`res`: the final residual,
// where the state's own is not the exact one) and the status it returns.
template <class S>
static cfd_status_t finish_stats(hip_proj_ctx* c, const S& s, double res) {
    c->pstats.status = (poisson_solver_status_t)s.status;
    c->pstats.iterations = s.iterations;
    c->pstats.initial_residual = s.res0;
    c->pstats.final_residual = res;
    return (s.status == ST_CONVERGED) ? CFD_SUCCESS : CFD_ERROR_MAX_ITER;
}
