// rt_host.hpp -- what EVERY translation unit of librtiow_hip.so shares: the context, the error path, parameter validation, the scene's
// fields of the kernel-argument block (set_scene_params), DeviceBlock (the one owner of a device buffer that grows with its use: ensure)
// and the plumbing of the host-buffer entry points: StageLayout / StagePlan / Stage (one device arena per context, laid out per call: a
// buffer is DECLARED once -- host pointer, element count, direction -- and its offset, its copies and its device pointer follow from that;
// there is no other way into the arena), timed_section (a pair of events of the call's own around its kernels) and grid_256.
// Also the argument checks the ray and path families share (rt_trace.hip, wavefront/rt_shade.hip, wavefront/rt_paths.hip): RT_NEED,
// check_no_flags / check_count / check_t_min / check_npix / check_frame_dims / check_context, and capped_grid and to_kcamera.
// rt_api.hip defines the functions declared here.  The render kernel is not among what is shared: this header takes its argument block
// from rt_params.hpp, and the units that launch it -- rt_api.hip, rt_frames.hip, rt_dense.hip -- add rt_launch.hpp.
// rt_scene_core.hpp (included here for rt_context's Header) builds the scene's tables on the host, pure and HIP-free; a change to what a
// table holds bumps its kTablesVersion and the static_assert on it in rt_api.hip, so that the hashed sources change with it.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>

#include "rtiow_hip.h"
#include "rt_params.hpp"
#include "rt_scene_core.hpp"
#include "rt_round_keys.hpp"
#ifdef RTIOW_CROSSCHECK_MODES
#include "xcheck/rt_xcheck_host_ctx.hpp"
#endif

namespace rt_host {
int fail(int code, const char *fmt, ...);          // records the thread's rt_last_error message, returns `code`
}

namespace rt_host {
// a device allocation a context owns, grows with ensure() and releases with itself (rt_destroy selects the device, then deletes the context)
struct DeviceBlock {
    void *ptr = nullptr; size_t bytes = 0;
    DeviceBlock() = default;
    DeviceBlock(const DeviceBlock &) = delete;
    DeviceBlock &operator=(const DeviceBlock &) = delete;
    ~DeviceBlock() { if (ptr) (void)hipFree(ptr); }
};
}

#define RT_HIP(call)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return rt_host::fail(e_ == hipErrorOutOfMemory ? RT_ERR_OUT_OF_MEMORY : RT_ERR_HIP,        \
                        "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

struct rt_context {
    int device = 0;
    int cu_count = 0;
    float *d_filt = nullptr;       // [n][4] f32 filter records (MODE 1)
    double *d_geo = nullptr;       // [n][4] exact geometry
    double *d_mat = nullptr;       // [n][kMatStride] exact materials
    uint4 *d_btube = nullptr;      // [tiles/2 + 1][64] MODE 5 (tube filter) B operands
    double *d_geo_slot = nullptr;  // MODE 5: [slots][4] exact geometry in table (slot) order
    uint32_t *d_slot_orig = nullptr;   // MODE 5: [slots] list index of the sphere in each column of the table
    rt_scene::Header scene;        // the scene's scalars: tile counts, the grid, the radius floor, the always-exact list (rt_scene_core.hpp)
#ifdef RTIOW_CROSSCHECK_MODES
    XcheckScene x;                 // device tables of scan modes 2-4 (xcheck/rt_xcheck_host_ctx.hpp)
#endif
    int scan_mode = 5;             // filter: 5 tube bf16x2 MFMA (default, shipped), 1 VALU + scalar loads (cross-check);
                                   // with -DRTIOW_CROSSCHECK_MODES also 2 f32 MFMA, 3 bf16x3 MFMA, 4 lifted bf16x3 MFMA
    int n_spheres = -1;
    // Per-launch state -- the work counter, the statistics words and the two events -- exists kSlots times, used in turn: a context
    // may have kSlots renders in flight (on different streams: the second fills the first one's end-of-launch tail); the fields
    // below name the slot of the LATEST launch, which is what rt_last_stats reports on.
    static constexpr int kSlots = 2;
    unsigned int *q_slots[kSlots] = {nullptr, nullptr};
    unsigned long long *s_slots[kSlots] = {nullptr, nullptr};
    hipEvent_t e0_slots[kSlots] = {nullptr, nullptr}, e1_slots[kSlots] = {nullptr, nullptr};
    bool slot_used[kSlots] = {false, false};
    int cur = 0;
    unsigned int *d_queue = nullptr;
    unsigned long long *d_stats = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipStream_t own_stream = nullptr;
    bool launched = false;
    unsigned long long zero_depth_samples = 0;
    rt_stats last{};
    // The staging arena of the host-buffer entry points (rt_host::Stage below): whatever the call in progress laid out in it, nothing
    // between calls.  Device-form entry points never touch it.
    rt_host::DeviceBlock arena;
    int blocks_per_cu = 0;     // 0 = occupancy query
    // rt_select_pixels_device's scratch (noisy / active flags, the workgroups' counts): a device form's, on the caller's stream, so not
    // in the arena -- rt_render_adaptive calls it while its own frame state lives there
    rt_host::DeviceBlock sel;
    int last_dense_body = 0;              // rt_last_dense_body (rtiow_hip_diag.h): 1 when the latest rt_render_device launch ran a capped-redraw kernel of rt_dense.hip, else 0
    int ring_min_spp = 0;                 // RTIOW_RING_MIN_SPP (diagnostic): spp per launch from which block sums are kept in LDS (0: the kernel's own minimum)
    // rt_render_wavefront_device's two path queues (wavefront/rt_paths.hip): a device form's, so not in the arena; allocated on first use,
    // regrown when a batch is larger
    rt_host::DeviceBlock paths;
};

namespace rt_host {

int validate_params(const rt_params *p);
// what a pixel-list render accepts beyond validate_params (rt_api.hip; the adaptive driver of rt_adaptive.hip asks it too)
int validate_pixel_list(const rt_context *ctx, const rt_camera *cam, const rt_params *p, int64_t n_pixels);
// the block holds at least `need` bytes: never shrunk; regrown by free + allocate, so contents are not preserved and the block may MOVE
int ensure(DeviceBlock &block, size_t need);
void set_scene_params(const rt_context *ctx, rt::KParams &kp);

// the grid of the element-wise kernels: 256 threads a block, at most 8 192 blocks (their grid-stride loops take the rest)
inline unsigned grid_256(long long n)
{
    const long long blocks = (n + 255) / 256;
    return (unsigned)(blocks > 8192 ? 8192 : blocks);
}

// Where the blocks of one host-form call lie in the arena: add(bytes) gives the byte offset of a new block.  Every block starts on a
// 256-byte boundary (what hipMalloc gives a buffer of its own; the kernels' 16-byte loads rely on it), in the order declared; a block
// of 0 bytes occupies nothing.  Pure arithmetic, no HIP call (tests/stage_layout_table.cpp tabulates it).
struct StageLayout {
    size_t total = 0;
    size_t add(size_t bytes)
    {
        const size_t offset = total;
        total += (bytes + 255) & ~(size_t)255;
        return offset;
    }
};

// What one host-form call declared, in declaration order: per buffer its block's offset (StageLayout::add, so a call that declares its
// buffers in a given order has the layout add() gives that order), its bytes, the caller's pointer and the direction.  A caller's pointer
// that is NULL declares a block of 0 bytes that is ABSENT: this is the one place where "optional buffer left out" is decided.  Fixed
// capacity, no heap: a declaration past kCapacity is remembered (overflow) and writes nothing.  Pure, no HIP call
// (tests/stage_layout_table.cpp tabulates it).
enum class StageDir : unsigned char { in, out, inout, scratch };
struct StagePlan {
    static constexpr int kCapacity = 16;
    struct Block { size_t offset, bytes; void *host; StageDir dir; };
    StageLayout layout;
    Block blocks[kCapacity];
    int n = 0;
    bool overflow = false;
    // the block's number, -1 past the capacity
    int declare(StageDir dir, const void *host, size_t bytes)
    {
        if (n == kCapacity) { overflow = true; return -1; }
        if (dir != StageDir::scratch && !host) bytes = 0;
        blocks[n] = {layout.add(bytes), bytes, const_cast<void *>(host), dir};
        return n++;
    }
    // the block has a device pointer: a scratch block, or a buffer the caller gave
    bool present(int k) const { return k >= 0 && k < n && (blocks[k].dir == StageDir::scratch || blocks[k].host); }
    // the block is copied before / after the call's kernels: upload() and download() take them in declaration order
    bool goes_up(int k) const { return present(k) && (blocks[k].dir == StageDir::in || blocks[k].dir == StageDir::inout); }
    bool comes_down(int k) const { return present(k) && (blocks[k].dir == StageDir::out || blocks[k].dir == StageDir::inout); }
};

// a declared buffer of elements T: only a name for the block -- its device pointer is Stage::ptr's to give, after commit()
template <class T> struct Staged { int block = -1; };

// One host-form call's use of the arena.  THE RULE: device-form entry points never touch the arena; a host-form entry point declares its
// buffers once, commits, and from then on calls only device forms -- so nothing can move or reuse a block while the call's work is in
// flight on own_stream.  in / out / inout(host, count) and scratch<T>(count) declare a buffer; commit() grows the arena to the call's
// total with ensure(), and the arena may MOVE when it grows, which is why a declaration returns a Staged and not a pointer.  After
// commit(): ptr(handle) is the device copy, nullptr for a buffer the caller left out; upload() copies every in and inout buffer the caller
// gave, download() every out and inout one, in declaration order (hipMemcpyAsync on ctx->own_stream); sync() waits for the stream;
// finish() is download() then sync(), the end of a host form that is not timed.  Sizes are element counts, stated where the buffer is
// declared and nowhere else.
class Stage {
public:
    explicit Stage(rt_context *ctx) : ctx_(ctx) {}
    template <class T> Staged<const T> in(const T *host, size_t count) { return {plan_.declare(StageDir::in, host, count * sizeof(T))}; }
    template <class T> Staged<T> out(T *host, size_t count) { return {plan_.declare(StageDir::out, host, count * sizeof(T))}; }
    template <class T> Staged<T> inout(T *host, size_t count) { return {plan_.declare(StageDir::inout, host, count * sizeof(T))}; }
    template <class T> Staged<T> scratch(size_t count) { return {plan_.declare(StageDir::scratch, nullptr, count * sizeof(T))}; }
    int commit()
    {
        if (plan_.overflow) return fail(RT_ERR_INVALID_ARGUMENT, "Stage: a call declared more than %d buffers", StagePlan::kCapacity);
        return ensure(ctx_->arena, plan_.layout.total);
    }
    template <class T> T *ptr(Staged<T> h) const { return plan_.present(h.block) ? reinterpret_cast<T *>(at(h.block)) : nullptr; }
    hipError_t upload() const
    {
        hipError_t he = hipSuccess;
        for (int k = 0; k < plan_.n && he == hipSuccess; ++k)
            if (plan_.goes_up(k)) he = hipMemcpyAsync(at(k), plan_.blocks[k].host, plan_.blocks[k].bytes, hipMemcpyHostToDevice, ctx_->own_stream);
        return he;
    }
    hipError_t download() const
    {
        hipError_t he = hipSuccess;
        for (int k = 0; k < plan_.n && he == hipSuccess; ++k)
            if (plan_.comes_down(k)) he = hipMemcpyAsync(plan_.blocks[k].host, at(k), plan_.blocks[k].bytes, hipMemcpyDeviceToHost, ctx_->own_stream);
        return he;
    }
    hipError_t sync() const { return hipStreamSynchronize(ctx_->own_stream); }
    hipError_t finish() const
    {
        const hipError_t he = download();
        return he == hipSuccess ? sync() : he;
    }
private:
    char *at(int k) const { return static_cast<char *>(ctx_->arena.ptr) + plan_.blocks[k].offset; }       // block k's device copy
    rt_context *ctx_;
    StagePlan plan_;
};

// Times what body() enqueues on ctx->own_stream with a pair of events of this call's own (the context's belong to its launch slots),
// created here and destroyed on every path: the first is recorded before body -- after the caller's uploads --, the second after it and
// before st.finish(), so *kernel_ms (may be NULL) covers the kernels only.  body returns a device form's code, which is passed on as it
// is with its own message; a HIP failure is "<name>: <error>".
template <class Body>
int timed_section(rt_context *ctx, const char *name, float *kernel_ms, const Stage &st, Body body)
{
    hipEvent_t e0 = nullptr, e1 = nullptr;
    RT_HIP(hipEventCreate(&e0));
    int rc = RT_OK;
    hipError_t he = hipEventCreate(&e1);
    if (he == hipSuccess) he = hipEventRecord(e0, ctx->own_stream);
    if (he == hipSuccess && !(rc = body())) {
        he = hipEventRecord(e1, ctx->own_stream);
        if (he == hipSuccess) he = st.finish();
        float ms = 0.0f;
        if (he == hipSuccess) he = hipEventElapsedTime(&ms, e0, e1);
        if (he == hipSuccess && kernel_ms) *kernel_ms = ms;
    }
    (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (rc) return rc;
    if (he != hipSuccess) return fail(RT_ERR_HIP, "%s: %s", name, hipGetErrorString(he));
    return RT_OK;
}

// ---- the argument checks the ray and path families share (rt_trace.hip, wavefront/rt_shade.hip, wavefront/rt_paths.hip).  An entry point
// runs the context-free ones first, then check_context, then selects the device.
#define RT_NEED(ptr, what, name) \
    do { if (!(ptr)) return rt_host::fail(RT_ERR_INVALID_ARGUMENT, "%s: %s is NULL", what, name); } while (0)

// noun: what the family calls itself ("the wavefront steps", "the path queue")
inline int check_no_flags(const char *what, uint32_t flags, const char *noun)
{
    if (flags & RT_FLAG_UNIFORM53)
        return fail(RT_ERR_INVALID_ARGUMENT, "%s: RT_FLAG_UNIFORM53 is not built for %s (flags 0x%x; only 0 is legal)", what, noun, flags);
    if (flags) return fail(RT_ERR_INVALID_ARGUMENT, "%s: unknown flags 0x%x (only 0 is legal)", what, flags);
    return RT_OK;
}
inline int check_count(const char *what, int64_t n)
{
    if (n < 0 || n > (int64_t)1 << 31) return fail(RT_ERR_INVALID_ARGUMENT, "%s: n must be in [0, 2^31] (is %lld)", what, (long long)n);
    return RT_OK;
}
inline int check_t_min(const char *what, double t_min)
{
    if (!(t_min > 0.0) || !std::isfinite(t_min)) return fail(RT_ERR_INVALID_ARGUMENT, "%s: t_min must be > 0 and finite (is %g)", what, t_min);
    return RT_OK;
}
inline int check_npix(const char *what, int64_t npix)
{
    if (npix <= 0 || npix > (int64_t)1 << 32) return fail(RT_ERR_INVALID_ARGUMENT, "%s: npix must be in [1, 2^32] (is %lld)", what, (long long)npix);
    return RT_OK;
}
inline int check_frame_dims(const char *what, int32_t width, int32_t height)
{
    if (width < 2 || height < 2) return fail(RT_ERR_INVALID_ARGUMENT, "%s: width and height must be >= 2 (are %d, %d)", what, width, height);
    return RT_OK;
}
// the context's part of every check, after the context-free ones
inline int check_context(const rt_context *ctx, const char *what, bool needs_mode5, bool needs_scene)
{
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (needs_mode5 && ctx->scan_mode != 5)
        return fail(RT_ERR_INVALID_ARGUMENT, "%s needs the shipped scan mode 5; this context was created under RTIOW_SCAN_MODE=%d", what, ctx->scan_mode);
    if (needs_scene && ctx->n_spheres < 0) return fail(RT_ERR_NO_SCENE, "rt_upload_scene has not been called");
    return RT_OK;
}

// a family's diagnostic knob <env_name>=k (read per call): at most k workgroups, so that a kernel's grid-stride trip runs at a test's size
inline long long capped_grid(const char *env_name, long long grid)
{
    const char *e = getenv(env_name);
    const long long cap = e && *e ? atoll(e) : 0;
    return cap > 0 && grid > cap ? cap : grid;
}

inline rt::KCamera to_kcamera(const rt_camera *cam)
{
    rt::KCamera kc;
    static_assert(sizeof(rt::KCamera) == sizeof(rt_camera), "camera layouts must match");
    memcpy(&kc, cam, sizeof(rt_camera));
    return kc;
}

} // namespace rt_host
