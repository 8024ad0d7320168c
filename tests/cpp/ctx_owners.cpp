// ctx_owners.cpp — who releases what inside rsreg_ctx (csrc/owned.hpp, csrc/rsreg_ctx.hpp), on a machine without a GPU:
// the HIP calls the owners make are defined HERE and count what they hand out.  A free or destroy of a handle that was
// never handed out, or handed back twice, aborts.  Built with -fsanitize=address,undefined by tests/test_ctx_owners_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>

#include "../../realsense-pointcloud_amd/csrc/rsreg_ctx.hpp"

namespace {

struct Ledger {
    std::set<void *> live;
    long made = 0;
    void *make()
    {
        void *p = std::malloc(16);
        live.insert(p);
        ++made;
        return p;
    }
    void give_back(void *p, const char *what)
    {
        if (!live.erase(p)) {
            std::fprintf(stderr, "%s of a handle that is not live: %p\n", what, p);
            std::abort();
        }
        std::free(p);
    }
};
std::mutex g_m;   // (a context's helper threads may call in here too)
Ledger g_dev, g_pinned, g_events, g_streams;
long g_creations = 0, g_fail_at = 0;   // the g_fail_at-th stream / event creation from now fails (0: none)

bool creation_fails() { return ++g_creations == g_fail_at; }
size_t live_total() { return g_dev.live.size() + g_pinned.live.size() + g_events.live.size() + g_streams.live.size(); }

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                             \
        }                                                                             \
    } while (0)

}  // namespace

extern "C" {
hipError_t hipMalloc(void **p, size_t) { std::lock_guard<std::mutex> lk(g_m); *p = g_dev.make(); return hipSuccess; }
hipError_t hipFree(void *p) { std::lock_guard<std::mutex> lk(g_m); g_dev.give_back(p, "hipFree"); return hipSuccess; }
hipError_t hipHostMalloc(void **p, size_t, unsigned int) { std::lock_guard<std::mutex> lk(g_m); *p = g_pinned.make(); return hipSuccess; }
hipError_t hipHostFree(void *p) { std::lock_guard<std::mutex> lk(g_m); g_pinned.give_back(p, "hipHostFree"); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned)
{
    std::lock_guard<std::mutex> lk(g_m);
    if (creation_fails()) return hipErrorOutOfMemory;
    *e = static_cast<hipEvent_t>(g_events.make());
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t *e) { return hipEventCreateWithFlags(e, 0); }
hipError_t hipEventDestroy(hipEvent_t e) { std::lock_guard<std::mutex> lk(g_m); g_events.give_back(e, "hipEventDestroy"); return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned)
{
    std::lock_guard<std::mutex> lk(g_m);
    if (creation_fails()) return hipErrorOutOfMemory;
    *s = static_cast<hipStream_t>(g_streams.make());
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) { std::lock_guard<std::mutex> lk(g_m); g_streams.give_back(s, "hipStreamDestroy"); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "stub"; }
}

namespace {

using namespace rsreg;

// moving a buffer leaves the source empty and frees once; a reserve within the capacity allocates nothing
template <typename Buf> void test_buffer(Ledger &led)
{
    const long made0 = led.made;
    {
        Buf a;
        CHECK(a.reserve(1000) == hipSuccess && a.ptr && a.cap == 1000 + 250 + 256);
        CHECK(led.made == made0 + 1 && led.live.size() == 1);
        void *p = a.ptr;
        CHECK(a.reserve(10) == hipSuccess && a.reserve(a.cap) == hipSuccess && a.ptr == p && led.made == made0 + 1);
        Buf b(std::move(a));
        CHECK(!a.ptr && !a.cap && b.ptr == p && b.cap == 1506 && led.live.size() == 1);
        Buf c;
        CHECK(c.reserve(8) == hipSuccess && led.live.size() == 2);
        c = std::move(b);   // (c's own allocation goes, b's moves in)
        CHECK(!b.ptr && !b.cap && c.ptr == p && led.live.size() == 1);
        CHECK(c.reserve(c.cap + 1) == hipSuccess && c.ptr != nullptr && led.live.size() == 1 && led.made == made0 + 3);   // growth: free, then allocate
        c.release();
        CHECK(!c.ptr && !c.cap && led.live.empty());
        c.release();
        CHECK(c.reserve(1) == hipSuccess);
    }
    CHECK(led.live.empty());
}

void test_handles()
{
    {
        Event e;
        CHECK(!e && e.ensure() == hipSuccess && e && g_events.live.size() == 1);
        const hipEvent_t h = e;
        CHECK(e.ensure() == hipSuccess && (hipEvent_t)e == h && g_events.live.size() == 1);
        Event f(std::move(e));
        CHECK(!e && (hipEvent_t)f == h);
        Stream s, t;
        CHECK(s.ensure() == hipSuccess && g_streams.live.size() == 1);
        t = std::move(s);
        CHECK(!s && t && g_streams.live.size() == 1);
        std::vector<Event> v;
        for (int k = 0; k < 9; ++k) {   // (the vector grows: moves, no copies, no double destroy)
            Event g;
            CHECK(g.ensure(hipEventDefault) == hipSuccess);
            v.push_back(std::move(g));
        }
        CHECK(g_events.live.size() == 10);
    }
    CHECK(live_total() == 0);
}

// a context with everything made: all of it is gone after delete
void test_context()
{
    rsreg_ctx *ctx = new rsreg_ctx();
    CHECK(ctx->src.ensure() == hipSuccess && ctx->up.ensure() == hipSuccess && ctx->down.ensure() == hipSuccess && ctx->h2d.ensure() == hipSuccess);
    for (auto &ss : ctx->side_sets) {
        CHECK(ss.stream.ensure() == hipSuccess);
        for (DevBuf *b : {&ss.out, &ss.keys, &ss.keys_alt, &ss.vals, &ss.vals_alt, &ss.flags, &ss.scan, &ss.cent, &ss.misc, &ss.tmp}) CHECK(b->reserve(64) == hipSuccess);
        CHECK(ss.host.reserve(64) == hipSuccess);
    }
    CHECK(ctx->ev_side_gate.ensure() == hipSuccess);
    for (Event &e : ctx->ev_ndt) CHECK(e.ensure(hipEventDefault) == hipSuccess);
    for (std::vector<Event> *v : {&ctx->ev_pool, &ctx->ev_home, &ctx->ev_copy})
        for (int k = 0; k < 5; ++k) {
            Event e;
            CHECK(e.ensure() == hipSuccess);
            v->push_back(std::move(e));
        }
    for (DevBuf *b : {&ctx->d_tgt_raw, &ctx->d_tgt_sorted, &ctx->d_dense, &ctx->d_misc, &ctx->d_cnt, &ctx->d_scan_keys, &ctx->d_smisc, &ctx->d_src, &ctx->d_sums,
                      &ctx->d_vox_out, &ctx->d_ndt_vox, &ctx->d_ndt_tgt, &ctx->d_fit_d2, &ctx->d_comm, &ctx->prep_model})
        CHECK(b->reserve(4096) == hipSuccess);
    for (PinnedBuf *b : {&ctx->h_smisc, &ctx->h_sums, &ctx->h_stage, &ctx->h2d.h_src, &ctx->h2d.h_tgt, &ctx->h_ndt, &ctx->h_ndt_build, &ctx->h_fit, &ctx->up.h[0],
                         &ctx->up.h[1], &ctx->down.h[0], &ctx->down.h[3]})
        CHECK(b->reserve(4096) == hipSuccess);
    for (PointGrid *g : {&ctx->fit_icp, &ctx->fit_ndt, &ctx->knn})
        for (DevBuf *b : {&g->d_pts, &g->d_start, &g->d_count, &g->d_mask, &g->d_scan, &g->d_box}) CHECK(b->reserve(128) == hipSuccess);
    for (DevBuf *b : {&ctx->filt.d_dist, &ctx->filt.d_flags, &ctx->filt.d_pos, &ctx->filt.d_sums, &ctx->filt.d_out}) CHECK(b->reserve(128) == hipSuccess);
    CHECK(ctx->filt.host.reserve(128) == hipSuccess);
    // the cloud pool: two buffers handed in, one taken out again and dropped by its new owner
    {
        DevBuf a, b, taken;
        CHECK(a.reserve(1 << 20) == hipSuccess && b.reserve(1 << 10) == hipSuccess);
        const size_t before = g_dev.live.size();
        ctx->cloud_pool.slots.push_back(std::move(a));
        ctx->cloud_pool.slots.push_back(std::move(b));
        CHECK(!a.ptr && !b.ptr && g_dev.live.size() == before);
        taken = std::move(ctx->cloud_pool.slots[0]);
        ctx->cloud_pool.slots[0] = std::move(ctx->cloud_pool.slots.back());
        ctx->cloud_pool.slots.pop_back();
        CHECK(taken.cap >= (1u << 20) && ctx->cloud_pool.slots.size() == 1 && ctx->cloud_pool.slots[0].ptr && g_dev.live.size() == before);
    }
    // the helper threads: each has run a job, none has been shut down by hand
    int ran = 0;
    ctx->src_worker.reset(new SourceWorker());
    ctx->src_worker->post([&] { ++ran; return 0; });
    CHECK(ctx->source_enqueued() == 0);
    ctx->up.worker.reset(new TicketWorker());
    CHECK(ctx->up.worker->wait(ctx->up.worker->post([&] { ++ran; return 0; })) == 0);
    for (auto &w : ctx->side_workers) {
        w.reset(new TicketWorker());
        CHECK(w->wait(w->post([&] { ++ran; return 0; })) == 0);
    }
    ctx->down.worker.reset(new DownloadWorker());
    char from[8] = "records", to[8] = {0};
    ctx->down.worker->wait_slot(0);
    ctx->down.worker->post(DownloadWorker::Job{nullptr, from, to, 8, 0, 0});
    CHECK(ctx->down.worker->wait_idle() == 0 && to[0] == 'r' && ran == 4);
    CHECK(!g_dev.live.empty() && !g_pinned.live.empty() && !g_events.live.empty() && g_streams.live.size() == 4 + rsreg_ctx::kSideSets);
    delete ctx;
    CHECK(g_dev.live.empty());
    CHECK(g_pinned.live.empty());
    CHECK(g_events.live.empty());
    CHECK(g_streams.live.empty());
}

// the k-th creation of a lane fails, for every k: the error comes back, the lane is empty, nothing is live, and the next
// ensure() makes the whole lane
template <typename Lane, typename Empty> void test_lane(int creations, Empty is_empty)
{
    for (int k = 1; k <= creations; ++k) {
        {
            Lane lane;
            g_creations = 0;
            g_fail_at = k;
            CHECK(lane.ensure() == hipErrorOutOfMemory);
            CHECK(g_creations == k);
            CHECK(is_empty(lane) && live_total() == 0);
            g_fail_at = 0;
            g_creations = 0;
            CHECK(lane.ensure() == hipSuccess && !is_empty(lane) && g_creations == creations);
            CHECK(g_streams.live.size() == 1 && (long)g_events.live.size() == creations - 1);
            CHECK(lane.ensure() == hipSuccess && g_creations == creations);   // (complete: nothing more is made)
        }
        CHECK(live_total() == 0);
    }
}

}  // namespace

int main()
{
    test_buffer<DevBuf>(g_dev);
    test_buffer<PinnedBuf>(g_pinned);
    test_handles();
    test_context();
    test_lane<rsreg_ctx::SourceLane>(3, [](const rsreg_ctx::SourceLane &l) { return !l.stream && !l.ev_done && !l.ev_main; });
    test_lane<rsreg_ctx::StageLane>(3, [](const rsreg_ctx::StageLane &l) { return !l.stream && !l.ev_src && !l.ev_tgt; });
    test_lane<rsreg_ctx::UploadLane>(4, [](const rsreg_ctx::UploadLane &l) { return !l.stream && !l.ev_gate && !l.ev[0] && !l.ev[1]; });
    test_lane<rsreg_ctx::DownloadLane>(2 + rsreg_ctx::DownloadLane::kSlots, [](const rsreg_ctx::DownloadLane &l) {
        bool none = !l.stream && !l.ev_gate;
        for (const Event &e : l.ev) none = none && !e;
        return none;
    });
    CHECK(live_total() == 0);
    std::printf("owners ok\n");
    return 0;
}
