// What every post-processing entry point shares (xfk_postproc.hip,
// xfk_magpost.hip, xfk_magpost_ac.hip): the scaffold around its body and the
// timer of the lab entry points.
#pragma once
#include "xfk_internal.h"

#include <algorithm>
#include <exception>
#include <string>
#include <vector>

namespace xfk {

// One post-processing entry point: refusals() names the problems the caller
// does not answer (XFK_OK: go on).  No C++ exception crosses the C boundary
// (the host tables allocate; the sorting workers catch their own), the
// problem's device and arena are active while body runs, and blocks retired
// meanwhile (scratch, the old block of a grown buffer) become reusable once
// the stream is idle, as at the end of a solve.
template <class R, class F>
int post_entry(xfk_problem *P, R &&refusals, F &&body)
{
    try {
        int rc = refusals();
        if (rc != XFK_OK) return rc;
        XFK_CHECK(hipSetDevice(P->device));
        {
            ArenaScope arena_scope(&P->arena);
            rc = body();
        }
        problem_recycle(P);
        return rc;
    } catch (const std::exception &e) {
        set_error(std::string("post-processing failed: ") + e.what());
        return XFK_ERR_ARG;
    } catch (...) {
        set_error("post-processing failed: unknown exception");
        return XFK_ERR_ARG;
    }
}

// f() between two events on the stream, repeats + 1 times (the first a warm-up): the median in ms
template <class F>
int timed_median(hipStream_t s, int repeats, F f, double &out)
{
    ScopedEvents<2> ev;
    XFK_CHECK(ev.create());
    std::vector<double> t;
    for (int k = 0; k <= repeats; ++k) {
        XFK_CHECK(hipEventRecord(ev[0], s));
        const int r = f();
        if (r != XFK_OK) return r;
        XFK_CHECK(hipEventRecord(ev[1], s));
        XFK_CHECK(hipEventSynchronize(ev[1]));
        float m = 0;
        XFK_CHECK(hipEventElapsedTime(&m, ev[0], ev[1]));
        if (k) t.push_back(m);
    }
    std::sort(t.begin(), t.end());
    out = t[t.size() / 2];
    return XFK_OK;
}

}  // namespace xfk
