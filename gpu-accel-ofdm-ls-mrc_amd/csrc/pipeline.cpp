// pipeline.cpp -- streaming ingest (include/ofdm_lsmrc.h, "streaming ingest";
// SURVEY.md 8(f) rank 2): host-resident IQ -> device -> fused receiver ->
// host outputs, with the two PCIe directions and the kernels overlapped.
//
// The reference moves one symbol at a time: readNextSymbolCUDA issues a
// cudaMemcpyAsync on a freshly created stream per symbol and the caller
// synchronises before the FFT (ShMemSymBuff_gpu.hpp:364-447, gpuLS.cu:351-473),
// so copy and compute never overlap and every 512 KiB symbol pays a launch +
// sync round trip.  Here a slot holds `chunk` whole frames; slot i's copy-in,
// compute and copy-out run on three streams ordered by events:
//
//   copy-in(i)  waits compute(i - depth)   (the slot's IQ buffer is free)
//   compute(i)  waits copy-in(i), copy-out(i - depth) (its output buffer is free)
//   copy-out(i) waits compute(i)
//
// so with depth >= 3 the H2D of chunk i+1, the kernels of chunk i and the D2H
// of chunk i-1 are in flight together.  No host thread blocks except in
// ofdm_pipeline_sync (and inside HIP when a host buffer is pageable).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <new>
#include <vector>

#include "../../include/ofdm_lsmrc.h"
#include "../../include/ofdm_lsmrc_acquire.h"
#include "../../include/ofdm_lsmrc_timing.h"
#include "launch.hpp"

struct ofdm_pipeline {
    struct Slot {
        void *iq = nullptr;          // chunk frames of ofdm_cf32, or of ofdm_sc16 (sc16 pipelines)
        ofdm_cf32 *f32 = nullptr;    // sc16 pipelines at C != 1024: the converted chunk
        ofdm_cf32 *out = nullptr;
        float *eps = nullptr;        // ofdm_pipeline_set_cfo: the chunk's per-frame offsets
        void *ws = nullptr;
        hipEvent_t in_done = nullptr, comp_done = nullptr, out_done = nullptr;
        bool used = false;       // has been submitted at least once
        bool acquired = false;   // acquire() called, submit() pending
    };
    int S = 0, R = 0, C = 0, cp = 0, K = 0, device = 0;
    bool sc16 = false;  // the slots hold ofdm_sc16 samples, x = i16 * scale
    float scale = 1.f;
    int taps_post = 0, taps_pre = 0;  // ofdm_pipeline_set_denoise; taps_post == 0: off
    bool cfo = false;                 // ofdm_pipeline_set_cfo
    int cp_skip = 0;
    int search = 0;                   // ofdm_pipeline_set_cfo_search; 0: off
    float search_ratio = 2.f;
    int phase_mod = 0;               // ofdm_pipeline_set_phase_track; 0: off
    int timing_mod = 0;              // ofdm_pipeline_set_timing_track; 0: off; set: runs instead of the phase tracker
    long long chunk = 0;
    size_t ws_bytes = 0, frame_in = 0, frame_out = 0;  // elements
    ofdm_cf32 *X = nullptr;
    hipStream_t s_in = nullptr, s_comp = nullptr, s_out = nullptr;
    std::vector<Slot> slots;
    int next = 0;
};

namespace {

int err(int code, const char *fn, const char *what) {
    char buf[384];
    std::snprintf(buf, sizeof buf, "%s: %s", fn, what);
    return ofdm::set_error(code, buf);
}

int herr(hipError_t e, const char *fn, const char *what) {
    if (e == hipSuccess) return OFDM_OK;
    char buf[384];
    std::snprintf(buf, sizeof buf, "%s: %s: %s", fn, what, hipGetErrorString(e));
    return ofdm::set_error(OFDM_E_HIP, buf);
}

bool positive_finite(float x) { return x > 0.f && x <= 3.402823466e38f; }

#define PL_TRY(expr, fn, what)                           \
    do {                                                 \
        int rc_ = herr((expr), fn, what);                \
        if (rc_) return rc_;                             \
    } while (0)

// Makes the pipeline's device current for the scope of a call and restores
// the caller's current device on every return path (a host thread driving
// pipelines on several GPUs keeps its own device selection).
struct DeviceGuard {
    int prev = -1;
    hipError_t e = hipSuccess;
    explicit DeviceGuard(int dev) {
        e = hipGetDevice(&prev);
        if (e == hipSuccess && prev != dev) e = hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

void release(ofdm_pipeline *p) {
    if (!p) return;
    DeviceGuard dg(p->device);
    for (auto &s : p->slots) {
        if (s.iq) (void)hipFree(s.iq);
        if (s.f32) (void)hipFree(s.f32);
        if (s.out) (void)hipFree(s.out);
        if (s.eps) (void)hipFree(s.eps);
        if (s.ws) {
            (void)ofdm_workspace_release(s.ws);  // its registry entry must not outlive the memory
            (void)hipFree(s.ws);
        }
        if (s.in_done) (void)hipEventDestroy(s.in_done);
        if (s.comp_done) (void)hipEventDestroy(s.comp_done);
        if (s.out_done) (void)hipEventDestroy(s.out_done);
    }
    if (p->X) (void)hipFree(p->X);
    if (p->s_in) (void)hipStreamDestroy(p->s_in);
    if (p->s_comp) (void)hipStreamDestroy(p->s_comp);
    if (p->s_out) (void)hipStreamDestroy(p->s_out);
    delete p;
}

// ofdm_pipeline_create / _create_sc16
int create(const char *fn, int S, int R, int C, int cp_len, bool sc16, float scale, const ofdm_cf32 *X,
           int chunk_frames, int depth, ofdm_pipeline **out) {
    if (!out || !X) return err(OFDM_E_ARG, fn, "null pointer");
    *out = nullptr;
    if (chunk_frames < 1 || depth < 1 || depth > 64)
        return err(OFDM_E_ARG, fn, "chunk_frames >= 1 and 1 <= depth <= 64 required");
    if (sc16 && !positive_finite(scale))
        return err(OFDM_E_ARG, fn, "sc16 samples need a positive finite scale");
    const size_t ws = ofdm_frame_workspace_bytes(chunk_frames, S, R, C);
    if (ws == 0) return err(OFDM_E_UNSUPPORTED, fn, "bad frame geometry (S >= 2, R >= 1, 2 <= C <= 8192)");
    if (cp_len < 0 || cp_len > C) return err(OFDM_E_ARG, fn, "cp_len out of [0, C]");
    auto *p = new (std::nothrow) ofdm_pipeline;
    if (!p) return err(OFDM_E_ARG, fn, "out of host memory");
    p->S = S; p->R = R; p->C = C; p->cp = cp_len; p->K = C - 1;
    p->chunk = chunk_frames;
    p->sc16 = sc16;
    p->scale = scale;
    p->ws_bytes = ws;
    p->frame_in = (size_t)S * R * (C + cp_len);
    p->frame_out = (size_t)(S - 1) * (C - 1);
    int rc;
#define CR(expr, what)                       \
    if ((rc = herr((expr), fn, what))) {     \
        release(p);                          \
        return rc;                           \
    }
    CR(hipGetDevice(&p->device), "hipGetDevice");
    CR(hipStreamCreateWithFlags(&p->s_in, hipStreamNonBlocking), "hipStreamCreate");
    CR(hipStreamCreateWithFlags(&p->s_comp, hipStreamNonBlocking), "hipStreamCreate");
    CR(hipStreamCreateWithFlags(&p->s_out, hipStreamNonBlocking), "hipStreamCreate");
    CR(hipMalloc(&p->X, (size_t)(C - 1) * sizeof(ofdm_cf32)), "hipMalloc(X)");
    CR(hipMemcpy(p->X, X, (size_t)(C - 1) * sizeof(ofdm_cf32), hipMemcpyDefault), "copy X");
    p->slots.resize(depth);
    for (auto &s : p->slots) {
        CR(hipMalloc(&s.iq, p->frame_in * chunk_frames * (sc16 ? sizeof(ofdm_sc16) : sizeof(ofdm_cf32))),
           "hipMalloc(iq slot)");
        if (sc16 && C != 1024)  // no sc16 receiver at this C: converted, then the fp32 one
            CR(hipMalloc(&s.f32, p->frame_in * chunk_frames * sizeof(ofdm_cf32)), "hipMalloc(fp32 slot)");
        CR(hipMalloc(&s.out, p->frame_out * chunk_frames * sizeof(ofdm_cf32)), "hipMalloc(out slot)");
        CR(hipMalloc(&s.ws, ws), "hipMalloc(workspace)");
        CR(hipEventCreateWithFlags(&s.in_done, hipEventDisableTiming), "hipEventCreate");
        CR(hipEventCreateWithFlags(&s.comp_done, hipEventDisableTiming), "hipEventCreate");
        CR(hipEventCreateWithFlags(&s.out_done, hipEventDisableTiming), "hipEventCreate");
    }
#undef CR
    *out = p;
    return OFDM_OK;
}

// an entry of one sample format (fmt_sc16: the caller's) on a pipeline of the other
int check_format(const char *fn, const ofdm_pipeline *p, bool fmt_sc16) {
    if (p->sc16 == fmt_sc16) return OFDM_OK;
    return err(OFDM_E_ARG, fn, p->sc16 ? "the pipeline holds sc16 samples (use the _sc16 entry)"
                                       : "the pipeline holds fp32 samples (use the entry without _sc16)");
}

// the acquire of either format
int acquire(const char *fn, ofdm_pipeline *p, bool fmt_sc16, void **d_iq, ofdm_stream_t *copy_stream) {
    if (!p || !d_iq) return err(OFDM_E_ARG, fn, "null pointer");
    if (int rc = check_format(fn, p, fmt_sc16)) return rc;
    auto &s = p->slots[p->next];
    if (s.acquired) return err(OFDM_E_ARG, fn, "slot already acquired: submit it first");
    DeviceGuard dg(p->device);
    PL_TRY(dg.e, fn, "hipSetDevice");
    // the copy into this slot must not overwrite IQ its previous compute still reads
    if (s.used) PL_TRY(hipStreamWaitEvent(p->s_in, s.comp_done, 0), fn, "hipStreamWaitEvent");
    s.acquired = true;
    *d_iq = s.iq;
    if (copy_stream) *copy_stream = reinterpret_cast<ofdm_stream_t>(p->s_in);
    return OFDM_OK;
}

// acquire + copy + submit over nframes host frames of `esize`-byte samples
int demod_all(const char *fn, ofdm_pipeline *p, bool fmt_sc16, const void *iq, size_t esize, long long nframes,
              ofdm_cf32 *out) {
    if (!p) return err(OFDM_E_ARG, fn, "null pipeline");
    if (nframes < 0 || (nframes > 0 && (!iq || !out))) return err(OFDM_E_ARG, fn, "bad arguments");
    if (int rc = check_format(fn, p, fmt_sc16)) return rc;
    for (long long f0 = 0; f0 < nframes; f0 += p->chunk) {
        const long long n = nframes - f0 < p->chunk ? nframes - f0 : p->chunk;
        void *d = nullptr;
        ofdm_stream_t cs = nullptr;
        int rc = acquire(fn, p, fmt_sc16, &d, &cs);
        if (rc) return rc;
        PL_TRY(hipMemcpyAsync(d, static_cast<const char *>(iq) + (size_t)f0 * p->frame_in * esize,
                              (size_t)n * p->frame_in * esize, hipMemcpyDefault, reinterpret_cast<hipStream_t>(cs)),
               fn, "copy-in");
        if ((rc = ofdm_pipeline_submit(p, n, out + (size_t)f0 * p->frame_out))) return rc;
    }
    return OFDM_OK;
}

// A chunk's sample source: which family of the public frame entries takes it.
// Plain: fp32 frames, every C.  Sc16: the slot's int16 frames; Cfo: fp32 frames
// and the slot's offsets; both have a receiver at C = 1024 only.  A new source
// is one more kind here and one more line in each of the three functions.
enum class Source { Plain, Sc16, Cfo };
using Slot = ofdm_pipeline::Slot;
const ofdm_sc16 *sc16_of(const Slot &s) { return static_cast<const ofdm_sc16 *>(s.iq); }

int estimate(Source src, const ofdm_pipeline &p, const Slot &s, const ofdm_cf32 *iq, long long n) {
    if (src == Source::Sc16)
        return ofdm_frame_estimate_sc16(sc16_of(s), n, p.S, p.R, p.C, p.cp, p.scale, p.X, s.ws, p.ws_bytes, p.s_comp);
    if (src == Source::Cfo)
        return ofdm_frame_estimate_cfo(iq, n, p.S, p.R, p.C, p.cp, p.X, s.ws, p.ws_bytes, s.eps, p.s_comp);
    return ofdm_frame_estimate(iq, n, p.S, p.R, p.C, p.cp, p.X, s.ws, p.ws_bytes, p.s_comp);
}
int combine(Source src, const ofdm_pipeline &p, const Slot &s, const ofdm_cf32 *iq, long long n) {
    if (src == Source::Sc16)
        return ofdm_frame_combine_sc16(sc16_of(s), n, p.S, p.R, p.C, p.cp, p.scale, s.ws, p.ws_bytes, s.out, p.s_comp);
    if (src == Source::Cfo)
        return ofdm_frame_combine_cfo(iq, n, p.S, p.R, p.C, p.cp, s.ws, p.ws_bytes, s.out, s.eps, p.s_comp);
    return ofdm_frame_combine(iq, n, p.S, p.R, p.C, p.cp, s.ws, p.ws_bytes, s.out, p.s_comp);
}
int demod(Source src, const ofdm_pipeline &p, const Slot &s, const ofdm_cf32 *iq, long long n) {
    if (src == Source::Sc16)
        return ofdm_frame_demod_sc16(sc16_of(s), n, p.S, p.R, p.C, p.cp, p.scale, p.X, s.ws, p.ws_bytes, s.out, p.s_comp);
    if (src == Source::Cfo)
        return ofdm_frame_demod_cfo(iq, n, p.S, p.R, p.C, p.cp, p.X, s.ws, p.ws_bytes, s.out, s.eps, p.s_comp);
    return ofdm_frame_demod(iq, n, p.S, p.R, p.C, p.cp, p.X, s.ws, p.ws_bytes, s.out, p.s_comp);
}

// The receiver of one chunk on the compute stream, a single chain: each step
// is written once and a new one goes in at its place in the order.
int receive(ofdm_pipeline *p, Slot &s, long long nframes) {
    // 1. an sc16 chunk at a C without an sc16 receiver: converted, then the fp32 forms
    int rc = OFDM_OK;
    if (s.f32) rc = ofdm_iq_convert_sc16(sc16_of(s), (long long)(nframes * p->frame_in), p->scale, s.f32, p->s_comp);
    if (rc) return rc;
    ofdm_cf32 *iq = s.f32 ? s.f32 : static_cast<ofdm_cf32 *>(s.iq);
    // 2. the chunk's offsets from its cyclic prefixes, then the integer part in
    // place on them; the derotating receiver takes them at C = 1024, at any
    // other C the chunk (the pipeline's own memory) is derotated in place
    const bool derotating = p->cfo && p->C == 1024;
    if (p->cfo) {
        rc = ofdm_frame_cfo_estimate(iq, nframes, p->S, p->R, p->C, p->cp, p->cp_skip, nullptr, s.eps, p->s_comp);
        if (rc == OFDM_OK && p->search > 0)
            rc = ofdm_frame_cfo_acquire(iq, nframes, p->S, p->R, p->C, p->cp, p->X, p->search, p->search_ratio, s.eps,
                                        s.eps, nullptr, nullptr, p->s_comp);
        if (rc == OFDM_OK && !derotating)
            rc = ofdm_frame_cfo_derotate(iq, iq, nframes, p->S, p->R, p->C, p->cp, s.eps, p->s_comp);
        if (rc) return rc;
    }
    // 3. the source
    const Source src = p->sc16 && !s.f32 ? Source::Sc16 : derotating ? Source::Cfo : Source::Plain;
    // 4. the receiver; with denoising, estimate -> denoise -> combine (the one-launch demod cannot take it in)
    if (p->taps_post > 0) {
        rc = estimate(src, *p, s, iq, nframes);
        if (rc == OFDM_OK)
            rc = ofdm_frame_estimate_denoise(s.ws, p->ws_bytes, nframes, p->S, p->R, p->C, p->taps_post, p->taps_pre,
                                             p->s_comp);
        if (rc == OFDM_OK) rc = combine(src, *p, s, iq, nframes);
    } else {
        rc = demod(src, *p, s, iq, nframes);
    }
    if (rc) return rc;
    // 5. a tracker, in place on the output, against the estimate step 4 left in the slot's workspace;
    // the timing tracker contains the phase tracker and runs in its place, not before it
    if (p->timing_mod)
        return ofdm_frame_timing_track(s.out, nframes, p->S, p->R, p->C, s.ws, p->ws_bytes, p->timing_mod, s.out,
                                       nullptr, nullptr, p->s_comp);
    if (p->phase_mod)
        return ofdm_frame_phase_track(s.out, nframes, p->S, p->R, p->C, s.ws, p->ws_bytes, p->phase_mod, s.out, nullptr,
                                      p->s_comp);
    return OFDM_OK;
}

// what ofdm_pipeline_set_phase_track / _set_timing_track refuse
int check_track(const char *fn, const ofdm_pipeline *p, int modulation) {
    if (!p) return err(OFDM_E_ARG, fn, "null pipeline");
    if (modulation != 0 && modulation != OFDM_MOD_QPSK && modulation != OFDM_MOD_QAM16 && modulation != OFDM_MOD_QAM64 &&
        modulation != OFDM_MOD_QAM256)
        return err(OFDM_E_ARG, fn, "modulation must be 0 (off), 2, 4, 6 or 8");
    return OFDM_OK;
}

}  // namespace

extern "C" {

int ofdm_pipeline_create(int S, int R, int C, int cp_len, const ofdm_cf32 *X, int chunk_frames,
                         int depth, ofdm_pipeline **out) {
    return create("ofdm_pipeline_create", S, R, C, cp_len, false, 1.f, X, chunk_frames, depth, out);
}

int ofdm_pipeline_create_sc16(int S, int R, int C, int cp_len, float scale, const ofdm_cf32 *X, int chunk_frames,
                              int depth, ofdm_pipeline **out) {
    return create("ofdm_pipeline_create_sc16", S, R, C, cp_len, true, scale, X, chunk_frames, depth, out);
}

int ofdm_pipeline_destroy(ofdm_pipeline *p) {
    if (!p) return OFDM_OK;
    const int rc = ofdm_pipeline_sync(p);
    release(p);
    return rc;
}

int ofdm_pipeline_acquire(ofdm_pipeline *p, ofdm_cf32 **d_iq, ofdm_stream_t *copy_stream) {
    return acquire("ofdm_pipeline_acquire", p, false, reinterpret_cast<void **>(d_iq), copy_stream);
}

int ofdm_pipeline_acquire_sc16(ofdm_pipeline *p, ofdm_sc16 **d_iq, ofdm_stream_t *copy_stream) {
    return acquire("ofdm_pipeline_acquire_sc16", p, true, reinterpret_cast<void **>(d_iq), copy_stream);
}

int ofdm_pipeline_submit(ofdm_pipeline *p, long long nframes, ofdm_cf32 *out) {
    static const char *fn = "ofdm_pipeline_submit";
    if (!p) return err(OFDM_E_ARG, fn, "null pipeline");
    auto &s = p->slots[p->next];
    if (!s.acquired) return err(OFDM_E_ARG, fn, "no acquired slot");
    if (nframes < 0 || nframes > p->chunk) return err(OFDM_E_ARG, fn, "nframes out of [0, chunk_frames]");
    DeviceGuard dg(p->device);
    // any failure below releases the slot (its frames are not demodulated) so
    // the pipeline stays usable: the next acquire hands out the same slot.
    // Once anything may have been enqueued on the compute stream for this slot
    // (from the wait on in_done on), the failure path still records
    // comp_done / out_done and marks the slot used (best effort), so that the
    // next acquire makes the copy-in wait for whatever kernel of this submit
    // is still reading the slot's IQ.
    struct Release {
        ofdm_pipeline *p;
        ofdm_pipeline::Slot &s;
        bool ok = false, enqueued = false;
        ~Release() {
            if (ok) return;
            if (enqueued) {
                (void)hipEventRecord(s.comp_done, p->s_comp);
                (void)hipStreamWaitEvent(p->s_out, s.comp_done, 0);
                (void)hipEventRecord(s.out_done, p->s_out);
                s.used = true;
            }
            s.acquired = false;
        }
    } rel{p, s};
    PL_TRY(dg.e, fn, "hipSetDevice");
    PL_TRY(hipEventRecord(s.in_done, p->s_in), fn, "hipEventRecord");
    rel.enqueued = true;
    PL_TRY(hipStreamWaitEvent(p->s_comp, s.in_done, 0), fn, "hipStreamWaitEvent");
    if (s.used) PL_TRY(hipStreamWaitEvent(p->s_comp, s.out_done, 0), fn, "hipStreamWaitEvent");
    if (int rc = nframes > 0 ? receive(p, s, nframes) : OFDM_OK) return rc;
    PL_TRY(hipEventRecord(s.comp_done, p->s_comp), fn, "hipEventRecord");
    PL_TRY(hipStreamWaitEvent(p->s_out, s.comp_done, 0), fn, "hipStreamWaitEvent");
    if (out && nframes > 0)
        PL_TRY(hipMemcpyAsync(out, s.out, p->frame_out * nframes * sizeof(ofdm_cf32),
                              hipMemcpyDefault, p->s_out),
               fn, "copy-out");
    PL_TRY(hipEventRecord(s.out_done, p->s_out), fn, "hipEventRecord");
    rel.ok = true;
    s.used = true;
    s.acquired = false;
    p->next = (p->next + 1) % (int)p->slots.size();
    return OFDM_OK;
}

int ofdm_pipeline_set_denoise(ofdm_pipeline *p, int taps_post, int taps_pre) {
    static const char *fn = "ofdm_pipeline_set_denoise";
    if (!p) return err(OFDM_E_ARG, fn, "null pipeline");
    if (taps_post < 0 || taps_pre < 0) return err(OFDM_E_ARG, fn, "taps_post >= 0 and taps_pre >= 0 required");
    if (taps_post == 0 && taps_pre != 0) return err(OFDM_E_ARG, fn, "taps_post == 0 (off) takes taps_pre == 0");
    if (taps_post > p->C - taps_pre) return err(OFDM_E_ARG, fn, "taps_post + taps_pre exceeds C");
    p->taps_post = taps_post;
    p->taps_pre = taps_pre;
    return OFDM_OK;
}

int ofdm_pipeline_set_cfo(ofdm_pipeline *p, int on, int cp_skip) {
    static const char *fn = "ofdm_pipeline_set_cfo";
    if (!p) return err(OFDM_E_ARG, fn, "null pipeline");
    if (!on) {
        p->cfo = false;
        return OFDM_OK;
    }
    if (p->cp == 0) return err(OFDM_E_ARG, fn, "cp_len == 0: the estimator needs a cyclic prefix");
    if (cp_skip < 0 || cp_skip >= p->cp) return err(OFDM_E_ARG, fn, "cp_skip out of [0, cp_len)");
    if (p->sc16 && p->C == 1024)
        return err(OFDM_E_UNSUPPORTED, fn, "an sc16 pipeline at C = 1024 has no derotating receiver");
    DeviceGuard dg(p->device);
    PL_TRY(dg.e, fn, "hipSetDevice");
    for (auto &s : p->slots)
        if (!s.eps) PL_TRY(hipMalloc(&s.eps, (size_t)p->chunk * sizeof(float)), fn, "hipMalloc(eps slot)");
    p->cfo = true;
    p->cp_skip = cp_skip;
    return OFDM_OK;
}

int ofdm_pipeline_set_cfo_search(ofdm_pipeline *p, int max_shift, float min_ratio) {
    static const char *fn = "ofdm_pipeline_set_cfo_search";
    if (!p) return err(OFDM_E_ARG, fn, "null pipeline");
    if (max_shift < 0 || max_shift > OFDM_ACQ_MAX_SHIFT)
        return err(OFDM_E_ARG, fn, "max_shift out of [0, OFDM_ACQ_MAX_SHIFT]");
    if (4 * max_shift > p->C) return err(OFDM_E_ARG, fn, "max_shift: the search needs 4 * max_shift <= C");
    if (!(min_ratio >= 1.f && positive_finite(min_ratio)))
        return err(OFDM_E_ARG, fn, "min_ratio: the gate needs a finite ratio >= 1");
    if (max_shift > 0 && p->C < 8) return err(OFDM_E_UNSUPPORTED, fn, "the search covers C in [8, 8192]");
    p->search = max_shift;
    p->search_ratio = min_ratio;
    return OFDM_OK;
}

int ofdm_pipeline_set_phase_track(ofdm_pipeline *p, int modulation) {
    if (int rc = check_track("ofdm_pipeline_set_phase_track", p, modulation)) return rc;
    p->phase_mod = modulation;
    return OFDM_OK;
}

int ofdm_pipeline_set_timing_track(ofdm_pipeline *p, int modulation) {
    if (int rc = check_track("ofdm_pipeline_set_timing_track", p, modulation)) return rc;
    p->timing_mod = modulation;
    return OFDM_OK;
}

int ofdm_pipeline_demod(ofdm_pipeline *p, const ofdm_cf32 *iq, long long nframes,
                        ofdm_cf32 *out) {
    return demod_all("ofdm_pipeline_demod", p, false, iq, sizeof(ofdm_cf32), nframes, out);
}

int ofdm_pipeline_demod_sc16(ofdm_pipeline *p, const ofdm_sc16 *iq, long long nframes, ofdm_cf32 *out) {
    return demod_all("ofdm_pipeline_demod_sc16", p, true, iq, sizeof(ofdm_sc16), nframes, out);
}

int ofdm_pipeline_sync(ofdm_pipeline *p) {
    static const char *fn = "ofdm_pipeline_sync";
    if (!p) return err(OFDM_E_ARG, fn, "null pipeline");
    DeviceGuard dg(p->device);
    PL_TRY(dg.e, fn, "hipSetDevice");
    PL_TRY(hipStreamSynchronize(p->s_in), fn, "sync copy-in");
    PL_TRY(hipStreamSynchronize(p->s_comp), fn, "sync compute");
    PL_TRY(hipStreamSynchronize(p->s_out), fn, "sync copy-out");
    return OFDM_OK;
}

int ofdm_host_register(void *ptr, size_t bytes) {
    if (!ptr || bytes == 0) return err(OFDM_E_ARG, "ofdm_host_register", "bad arguments");
    return herr(hipHostRegister(ptr, bytes, hipHostRegisterDefault), "ofdm_host_register",
                "hipHostRegister");
}

int ofdm_host_unregister(void *ptr) {
    if (!ptr) return err(OFDM_E_ARG, "ofdm_host_unregister", "null pointer");
    return herr(hipHostUnregister(ptr), "ofdm_host_unregister", "hipHostUnregister");
}

}  // extern "C"
