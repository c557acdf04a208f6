// The frame of one host-side call of the SfM stages (K31-K37) and of the ring batches (K16-K24); included by pvlm_internal.h.  An entry point declares one pvlm_call, enters, and does its device
// work through it: scratch, queued copies, memsets and launches all stop at the first error, which `st` keeps.  The frame owns the rule that used to be an
// instruction to every caller: scratch and staged copies never outlive the call.  Its destructor waits for whatever is still queued (an error path that left
// before its sync), DROPS the staged device-to-host copies instead of landing them (their targets are locals of the returning function, some destroyed already),
// and only then hands the scratch back to the pool.  A result therefore reaches the caller only through sync().
#pragma once
#include <cstdlib>

struct pvlm_call {
  pvlm_ctx* ctx; const char* who;
  pvlm_status st = PVLM_OK;            // the first error of the call
  bool queued = false;                 // something went on the stream or into the staging arena since the last sync
  pvlm_dev_scratch tmp;                // destroyed after the destructor's body: the blocks go back behind the wait
  pvlm_call(pvlm_ctx* c, const char* w) : ctx(c), who(w), tmp(c) {}
  ~pvlm_call() { if (queued) { ctx->stage.deferred.clear(); (void)pvlm_i_sync(ctx); } }
  pvlm_call(const pvlm_call&) = delete;
  pvlm_call& operator=(const pvlm_call&) = delete;

  // binds the device; no entry point of these stages can be captured (they allocate, stage copies and synchronise)
  pvlm_status enter() {
    if (pvlm_i_bind(ctx)) return st = PVLM_ERR_HIP;
    if (ctx->capturing) { PVLM_SET_ERR(ctx, "%s inside a graph capture", who); return st = PVLM_ERR_STATE; }
    return PVLM_OK;
  }
  // count elements of scratch (0: a valid block of one), nullptr after an error
  template <class T> T* alloc(size_t count) { T* p = nullptr; if (!st) st = tmp.alloc(&p, count); return p; }
  // scratch of count elements with the upload of src queued behind it (count 0: the block without a copy)
  template <class T> T* upload(const T* src, size_t count) { T* p = alloc<T>(count); h2d(p, src, count * sizeof(T)); return p; }
  // The scratch taken while a `batch` lives goes back when it dies (the body of a loop over batches): the pool is stream-ordered, so the next batch may be
  // handed the same blocks behind this one's kernels.
  struct batch {
    pvlm_call& c; size_t mark;
    explicit batch(pvlm_call& call) : c(call), mark(call.tmp.ptrs.size()) {}
    ~batch() { for (size_t i = mark; i < c.tmp.ptrs.size(); ++i) pvlm_i_free(c.ctx, c.tmp.ptrs[i]); c.tmp.ptrs.resize(mark); }
  };
  // copies through the staging arena: an upload has left src when it returns, a download reaches dst at the next sync()
  void h2d(void* dst, const void* src, size_t bytes) { if (!st && bytes) { queued = true; st = pvlm_i_h2d_q(ctx, dst, src, bytes); } }
  void d2h(void* dst, const void* src, size_t bytes) { if (!st && bytes) { queued = true; st = pvlm_i_d2h_q(ctx, dst, src, bytes); } }
  // a large copy that does not go through the arena: its host side is pinned memory the caller owns, `s` the context's stream or a second one the caller drains
  void copy_pinned(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
    if (st || !bytes) return;
    queued = true;
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, s);
    if (e != hipSuccess) { PVLM_SET_ERR(ctx, "%s: copy failed: %s", who, hipGetErrorString(e)); st = e == hipErrorOutOfMemory ? PVLM_ERR_NOMEM : PVLM_ERR_HIP; }
  }
  void memset(void* dst, int value, size_t bytes) {
    if (st || !bytes) return;
    queued = true;
    if (hipMemsetAsync(dst, value, bytes, ctx->stream) != hipSuccess) { PVLM_SET_ERR(ctx, "%s: memset failed", who); st = PVLM_ERR_HIP; }
  }
  // a kernel on the context's stream; check_launches() after a launch or a group of launches
  template <class... P, class... A> void launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds_bytes, A... args) {
    if (st) return;
    queued = true;
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, ctx->stream, args...);
  }
  pvlm_status check_launches() {
    if (st) return st;
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { PVLM_SET_ERR(ctx, "%s: kernel launch failed: %s", who, hipGetErrorString(e)); st = PVLM_ERR_HIP; }
    return st;
  }
  // waits for the stream and lands the staged downloads; returns the first error of the call
  pvlm_status sync() {
    const pvlm_status s = pvlm_i_sync(ctx);
    queued = false;
    if (!st) st = s;
    return st;
  }
};

// A batch limit that an environment variable may lower (read at every call): min(deflt, v) for a value v > 0, deflt for anything else.  How the tests cross batch
// boundaries on small inputs; it changes no result.
inline long long pvlm_i_env_limit(const char* name, long long deflt) {
  const char* e = std::getenv(name);
  const long long v = e ? std::atoll(e) : 0;
  return v > 0 && v < deflt ? v : deflt;
}
