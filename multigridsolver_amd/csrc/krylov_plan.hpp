// krylov_plan.hpp — what the Krylov plans share (pcg_plan.hip, bicgstab_plan.hip, fgcr_plan.hip): the device block of work vectors with the
// state behind them, the ring of posted slots in mapped host memory with the wait on it, the checks of create and of every call, result and
// info.  Each plan's state struct, step kernel, vector passes and launch decisions stay in its own file: they pin its bits to its host solver.
#pragma once
#include <chrono>
#include <time.h>

#include "blas1.hpp"
#include "krylov_lookahead.hpp"

namespace krylov {
using blas1::vd2; using blas1::st2; using blas1::al16; using blas1::nts_of;      // the vector passes end in BLAS1_FOLD1 / BLAS1_FOLD2
constexpr int PTB = blas1::TB;           // lanes per workgroup of the vector passes
constexpr int RED = MGS_DOT_BLOCKS;      // red_dev[RED], red_dev[RED + 1]: what the last fold left

// What a posting step leaves for the host.  aux0, aux1: fields of the state that only its own plan reads (mgs_fgcr_plan: why, m_open), or 0
struct Slot {      // 64 bytes of mapped host memory
  unsigned long long ticket;
  double resid, normb;
  int it, status, frozen, wasted, aux0, aux1;
  unsigned long long pad[2];
};
static_assert(sizeof(Slot) == 64, "one slot per 64 bytes");
struct Look { int it, status, frozen, wasted, aux0, aux1; double resid, normb; };

template <class State>
__device__ __forceinline__ void post_slot(Slot *s, const State *st, unsigned long long ticket, const int *aux0 = nullptr, const int *aux1 = nullptr) {
  __hip_atomic_store(&s->resid, st->resid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&s->normb, st->normb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&s->it, st->it, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&s->status, st->status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&s->frozen, st->frozen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&s->wasted, st->wasted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&s->aux0, aux0 ? *aux0 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&s->aux1, aux1 ? *aux1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&s->ticket, ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// State: the plan's state block; it has it, status, frozen, wasted, resid, true_resid and normb among its fields.
template <class State>
struct Plan {
  const char *name = "";              // "mgs_pcg_plan", ...: the head of the messages of wait_post
  mgs_ctx *ctx = nullptr;
  const mgs_csr *A = nullptr;
  mgs_hier *h = nullptr;
  bool ns = false;
  int n = 0;
  double *block = nullptr;            // the work vectors (stride doubles each), then the state
  int64_t stride = 0, bytes = 0;
  State *st = nullptr;
  Slot *ring = nullptr, *ring_dev = nullptr;          // RING slots, then one State the result is copied into (mapped, coherent host memory)
  State *snap = nullptr;
  unsigned long long seq = 0;         // ticket of the last posting step enqueued
  // what info and result report
  int64_t calls = 0, enq_iters = 0, wasted = 0, waits = 0, restarts = 0;
  bool unread = false;                // an enqueue whose result has not been read yet
  int res_it = 0, res_status = 1; double res_resid = 0.0, res_rec = 0.0;

  // create: a square unsharded operator, a finalized hierarchy of the same kind on the same context
  int validate(const mgs_csr *A_, mgs_hier *h_, const char *who, const char *served_by) {
    MGS_TRY(mgs_check_unsharded(A_, h_, who, served_by));
    mgs_ctx *c = A_->ctx;
    ctx = c; A = A_; h = h_; n = A_->rows;
    return MGS_OK;
  }
  // create, behind validate: the null-space rule, then nvec vectors (256-byte aligned) and the state in one zeroed device block, and the host ring
  int allocate(const char *who, int nvec, bool serves_fields = false) {
    MGS_TRY(mgs_krylov_nullspace(A, h, who, &ns, serves_fields));
    MGS_TRY(mgs_csr_optimize(const_cast<mgs_csr *>(A)));
    stride = (((int64_t)n + 31) / 32) * 32;
    const size_t nstate = (sizeof(State) + 255) / 256 * 32;                                // doubles
    const size_t ndoubles = (size_t)nvec * stride + nstate;
    MGS_TRY(mgs_dev_alloc(ctx, &block, ndoubles));
    if (hipMemsetAsync(block, 0, sizeof(double) * ndoubles, ctx->stream) != hipSuccess) return mgs_fail(ctx, MGS_ERR_HIP, "%s: hipMemsetAsync failed", who);
    const size_t hb = sizeof(Slot) * RING + (sizeof(State) + 255) / 256 * 256;
    if (hipHostMalloc((void **)&ring, hb, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) { ring = nullptr; return mgs_fail(ctx, MGS_ERR_ALLOC, "%s: mapped host ring", who); }
    memset(ring, 0, hb);
    snap = reinterpret_cast<State *>(ring + RING);
    if (hipHostGetDevicePointer((void **)&ring_dev, ring, 0) != hipSuccess) return mgs_fail(ctx, MGS_ERR_HIP, "%s: the host ring is not mappable into the device", who);
    st = reinterpret_cast<State *>(block + (int64_t)nvec * stride);
    bytes = (int64_t)(sizeof(double) * ndoubles);
    return MGS_OK;
  }
  mgs_vec view(int k) const { mgs_vec v; v.ctx = ctx; v.n = n; v.d = block + (int64_t)k * stride; v.owns = false; return v; }
  // destroy: waits for the stream, then frees the block and the ring
  void release() {
    if (block || ring) hipStreamSynchronize(ctx->stream);
    if (block) mgs_hip_free(block);
    if (ring) hipHostFree(ring);
    block = nullptr; ring = nullptr;
  }

  // a step launch: the slot it posts into, with the next ticket in seq (post = false: NULL, seq as it is)
  Slot *next_slot(bool post) { return post ? ring_dev + (++seq % RING) : nullptr; }
  // wait until the post with ticket `want` is visible (no slot is rewritten before it has been read: see RING)
  int wait_post(unsigned long long want, Look *out) {
    Slot *s = ring + (want % RING);
    waits++;
    const auto t0 = std::chrono::steady_clock::now();
    double next_query = 2e-3;
    for (;;) {
      if (__atomic_load_n(&s->ticket, __ATOMIC_ACQUIRE) == want) break;
      const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (waited < 300e-6) { for (int k = 0; k < 8; ++k) __builtin_ia32_pause(); continue; }
      if (waited > next_query) {           // a queue that has drained (or failed) without the ticket will never deliver it
        next_query = waited + 2e-3;
        const hipError_t e = hipStreamQuery(ctx->stream);
        if (e == hipSuccess) {
          if (__atomic_load_n(&s->ticket, __ATOMIC_ACQUIRE) == want) break;
          return mgs_fail(ctx, MGS_ERR_HIP, "%s: posted results never reached the host ring", name);
        }
        if (e != hipErrorNotReady) return mgs_fail(ctx, MGS_ERR_HIP, "%s: %s", name, hipGetErrorString(e));
      }
      struct timespec ts = {0, 25000}; nanosleep(&ts, nullptr);
    }
    out->it = s->it; out->status = s->status; out->frozen = s->frozen; out->wasted = s->wasted; out->aux0 = s->aux0; out->aux1 = s->aux1;
    out->resid = s->resid; out->normb = s->normb;
    return MGS_OK;
  }

  int check_call(const mgs_vec *x, const mgs_vec *b, const char *who) {
    MGS_CHECK(ctx, x->n >= n && b->n >= n, MGS_ERR_INVALID, "%s: vectors of %lld and %lld entries, the operator has %d rows", who, (long long)x->n, (long long)b->n, n);
    MGS_CHECK(ctx, x->d != b->d, MGS_ERR_INVALID, "%s: x must not alias b", who);
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    MGS_HIP(ctx, hipStreamIsCapturing(ctx->stream, &cs));
    MGS_CHECK(ctx, cs == hipStreamCaptureStatusNone, MGS_ERR_STATE, "%s: the context's stream is being captured", who);
    return MGS_OK;
  }
  // behind check_call: views of n entries onto x and b, the counters of a new call
  void begin_call(const mgs_vec *x, const mgs_vec *b, mgs_vec *xv, mgs_vec *bv, bool unread_) {
    xv->ctx = bv->ctx = ctx; xv->n = bv->n = n; xv->d = x->d; bv->d = b->d; xv->owns = bv->owns = false;
    calls++; enq_iters = 0; wasted = 0; waits = 0; restarts = 0; unread = unread_;
  }
  // the state as the stream has left it, into host memory (asynchronous)
  int snapshot() {
    MGS_HIP(ctx, hipMemcpyAsync(snap, st, sizeof(State), hipMemcpyDeviceToHost, ctx->stream));
    return MGS_OK;
  }
  // of the last call; behind an enqueue it waits for the stream and reads the snapshot.  recursive_resid may be NULL
  int result(const char *who, int *iters_done, double *resid, double *recursive_resid, int *status) {
    MGS_CHECK(ctx, calls > 0, MGS_ERR_STATE, "%s: nothing has been solved or enqueued", who);
    if (unread) {
      MGS_HIP(ctx, hipStreamSynchronize(ctx->stream));
      res_it = snap->it; res_status = snap->status; res_resid = snap->true_resid; res_rec = snap->resid; wasted = snap->wasted;
      unread = false;
    }
    if (iters_done) *iters_done = res_it;
    if (resid) *resid = res_resid;
    if (recursive_resid) *recursive_resid = res_rec;
    if (status) *status = res_status;
    return MGS_OK;
  }
  void info(int64_t out[6]) const { out[0] = bytes; out[1] = calls; out[2] = enq_iters; out[3] = wasted; out[4] = waits; out[5] = restarts; }
};
}   // namespace krylov
