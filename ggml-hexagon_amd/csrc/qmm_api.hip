// qmm_api.hip — host side of the C-ABI declared in include/ggml_mi355x_qmm.h.
// gfx950 only; there is no CPU path: every failure is reported, nothing is silently emulated.

#include "qmm_host.h"

#include "qmm_matvec.hiph"
#include "qmm_mfma.hiph"              // the prefill kernels ...
#include "qmm_mfma_regb.hiph"
#include "qmm_mfma_r64s.hiph"
#include "qmm_prefill.hiph"           // ... and, behind them, what launches them
#include "qmm_moe.hiph"
#include "qmm_chain.hiph"
#include "qmm_bf16.hiph"              // BF16 weights: kernels, and the executor of qmm_bf16_plan.h

using namespace qmm;

template <int T>
static int launch_dequant(hipStream_t st, const void * w, int64_t rb, int64_t rows, int64_t K, float * dst) {
    const int64_t n = rows * (K / Traits<T>::UNIT_W);
    if (n == 0) return QMM_OK;
    hipLaunchKernelGGL((dequant_kernel<T>), dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, st,
                       (const uint8_t *) w, rb, rows, (int) K, dst);
    HIP_TRY(hipGetLastError());
    return QMM_OK;
}

static_assert(QMM_MATVEC_MAX_N == 8, "QMM_FOR_NTOK lists the token counts");

static MatvecRules matvec_rules(const qmm_ctx * c) { return { c->cus, c->mv_bpc, c->mv_kmix, c->mv_onepass, c->act_mode }; }

// the executor of every few-token launch (group calls and chain steps that go out on their own): the plan's instantiation on g
static int run_matvec(qmm_ctx * c, hipStream_t st, const MatvecLaunch & l, const MatvecGroup & g, const float * x, int64_t ldx) {
    char text[96];
    if (l.error) { l.text(text, sizeof(text)); return fail(l.error, "%s", text); }
    const MatvecKernel kern = qmm_internal_matvec_kernel(l);           // (qmm_matvec.hip holds the instantiations)
    if (!kern) return fail(QMM_EINVAL, l.kind == MV_PER_TYPE ? "matvec: N=%d" : "kmix matvec: N=%d", l.ntok);
    if (l.lds > 64 * 1024) HIP_TRY(hipFuncSetAttribute((const void *) kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int) l.lds));
    if (c->trace) { l.text(text, sizeof(text)); QMM_TRACE(c, "%s", text); }
    hipLaunchKernelGGL(kern, dim3(l.blocks), dim3(l.waves * WAVE), l.lds, st, x, ldx, l.K, l.act_arg, g.row_end[g.n - 1], g);
    HIP_TRY(hipGetLastError());
    return QMM_OK;
}

// matrices idx[0 .. n - 1] of a call (cumulative rows row_end) from token n0 on, with what the caller folds in, as the kernels' argument
static MatvecGroup matvec_group(const qmm_weight * ws, const int * idx, const int * row_end, int n, int64_t n0, const qmm_mv_extra * ex) {
    MatvecGroup g;
    memset(&g, 0, sizeof(g));
    for (int m = 0; m < n; ++m) {
        const qmm_weight & w = ws[idx[m]];
        g.w[m] = (const uint8_t *) w.w;  g.dst[m] = w.dst + n0 * w.ldd;  g.row_bytes[m] = w.w_row_bytes;  g.ldd[m] = w.ldd;
        g.type[m] = w.type;
        g.row_end[m] = row_end[m];
        if (ex && ex->residual[idx[m]]) g.res[m] = ex->residual[idx[m]] + n0 * w.ldd;
    }
    g.n = n;
    if (ex) { g.norm_w = ex->norm_w; g.norm_eps = ex->norm_eps; g.swiglu = ex->swiglu; }
    return g;
}

static int check_mm(const qmm_ctx * c, int type, const void * w, int64_t rb, int64_t K, const float * x, int64_t ldx, const char * who) {
    if (!type_known(type)) return fail(QMM_EUNSUPPORTED, "%s: type %d not supported", who, type);
    if (const int rc = need_codebook(c, type, who)) return rc;
    if (K <= 0 || K % type_blck(type)) return fail(QMM_EUNSUPPORTED, "%s: K=%lld must be a multiple of %d", who, (long long) K, type_blck(type));
    if (rb < (int64_t) qmm_row_size(type, K)) return fail(QMM_EINVAL, "%s: weight row stride %lld < row size", who, (long long) rb);
    if (iq1m_misaligned(type, w, rb)) return fail(QMM_EINVAL, "%s: IQ1_M rows must be 8-byte aligned (base address and row stride multiples of 8)", who);
    if ((uintptr_t) x % 16 || ldx % 4 || ldx < K) return fail(QMM_EINVAL, "%s: src1 must be 16-byte aligned with ldx %% 4 == 0", who);
    if (type_planar(type) && (!qmm_planar_type(type_base(type), K, rb) || (uintptr_t) w % 16))
        return fail(QMM_EINVAL, "%s: planar type %d wants 16-byte aligned rows and K a multiple of %d", who, type, type_base(type) == T_Q6_K ? 2048 : 256);
    return QMM_OK;
}


// ------------------------------------------------------------------------------------------- chains (qmm_chain.hiph)

static size_t chain_step_lds(const ChainStep & st, int ntok) {
    return chain_act_bytes(st.fam, ntok, st.K) + (st.g.norm_w ? (size_t) ntok * st.K * 4 : 0);
}
constexpr size_t CHAIN_SLAB = (size_t) CHAIN_RPW * CHAIN_NW * 4;          // one token

// the step as a launch of its own (a chain of one, or chains switched off): the kernels of round 1
static int chain_step_plain(qmm_ctx * c, hipStream_t st, const ChainStep & s) {
    const MatvecLaunch l = matvec_launch(matvec_rules(c), mv_kind_of(s.g.type, s.g.n), s.g.type[0], nullptr, s.g.row_end, s.g.n, s.K, 0, 1, s.g.norm_w != nullptr, s.g.swiglu, s.g.res);
    return run_matvec(c, st, l, s.g, s.x, s.ldx);
}

static int chain_launch(qmm_ctx * c) {
    if (!c->chain || c->chain->empty()) return QMM_OK;
    std::vector<ChainStep> & v = *c->chain;
    hipStream_t st = c->chain_stream;
    int rc = QMM_OK;
    for (size_t i = 0; i < v.size() && rc == QMM_OK;) {
        size_t n = v.size() - i;
        if (n > (size_t) CHAIN_MAX_STEPS) n = CHAIN_MAX_STEPS;
        if (n == 1) {
            rc = chain_step_plain(c, st, v[i]);
        } else {
            ChainArgs a;
            memset(&a, 0, sizeof(a));
            size_t lds = 0;
            for (size_t k = 0; k < n; ++k) {
                a.s[k] = v[i + k];
                const size_t b = chain_step_lds(a.s[k], 1);
                if (b > lds) lds = b;
            }
            a.sync = c->chain_sync;
            a.n = (int) n;
            a.act_mode = c->act_mode;
            a.timeout = 2000000u;                                           // 20 ms of the 100 MHz clock
            a.res_off = (uint32_t) ((lds + 15) & ~(size_t) 15);
            if (c->chain_dbg) {                                             // diagnostic stamps, consecutive launches behind each other
                a.dbg = c->chain_dbg;
                c->chain_dbg += n * (size_t) c->cus * 8;
            }
            const size_t total = a.res_off + CHAIN_SLAB;
            auto kern = matvec_chain_kernel<1>;
            if (!c->chain_attr_set) {
                hipError_t e = hipFuncSetAttribute((const void *) kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int) MV_LDS_LAUNCH - 256);
                if (e != hipSuccess) { rc = fail(QMM_EHIP, "chain: hipFuncSetAttribute: %s", hipGetErrorString(e)); break; }
                c->chain_attr_set = true;
            }
            QMM_TRACE(c, "matvec_chain_kernel<1>");
            hipLaunchKernelGGL(kern, dim3(c->cus), dim3(CHAIN_NW * WAVE), total, st, a);
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) { rc = fail(QMM_EHIP, "chain launch: %s", hipGetErrorString(e)); break; }
            c->chain_launches++;
            c->chain_steps += (int) n;
        }
        i += n;
    }
    v.clear();
    return rc;
}

// Record one group call (one token) as one step per activation format.  Returns 1 when recorded, 0 when the call is not eligible
// (the caller flushes and launches it the ordinary way), < 0 on error.
static int chain_record(qmm_ctx * c, hipStream_t st, const qmm_weight * ws, int nw, int64_t K, const float * x, int64_t ldx, const qmm_mv_extra * ex) {
    if (nw > MV_MAX_GROUP) return 0;
    const int W = c->cus * CHAIN_NW;
    int fams[2] = { 0, 0 };
    int64_t rows = 0;
    for (int i = 0; i < nw; ++i) {
        if (ws[i].M <= 0) return 0;
        if (chain_family(ws[i].type) == CHAIN_FAM_NONE) return 0;
        fams[chain_family(ws[i].type)]++;
        rows += ws[i].M;
        // a result on top of the activations is a race between workgroups in any launch form: leave it to the caller's order
        const char * d0 = (const char *) ws[i].dst, * x0 = (const char *) x;
        if (d0 < x0 + K * 4 && x0 < d0 + ws[i].M * 4) return 0;
    }
    if (fams[1] && K % 256) return 0;
    if ((rows + W - 1) / W > CHAIN_RPW) return 0;
    if (ex && ex->swiglu && fams[0] && fams[1]) return 0;
    if (!chain_step_fits(fams[1] ? CHAIN_FAM_Q8_K : CHAIN_FAM_Q8_0, K, ex && ex->norm_w, CHAIN_SLAB)) return 0;
    if (c->chain->empty()) c->chain_stream = st;
    else if (c->chain_stream != st) { int rc = chain_launch(c); if (rc) return rc; c->chain_stream = st; }
    bool first = true;
    for (int fam = 1; fam >= 0; --fam) {
        if (!fams[fam]) continue;
        ChainStep s;
        memset(&s, 0, sizeof(s));
        int n = 0, r = 0, idx[MV_MAX_GROUP], row_end[MV_MAX_GROUP];
        for (int i = 0; i < nw; ++i)
            if (chain_family(ws[i].type) == fam) { idx[n] = i; row_end[n++] = r += (int) ws[i].M; }
        s.g = matvec_group(ws, idx, row_end, n, 0, ex);
        s.x = x;  s.ldx = ldx;  s.K = (int) K;  s.fam = fam;
        s.dep = first ? 1 : 0;                          // the second format of one call reads the same x and writes other rows
        s.restage = 1;
        first = false;
        c->chain->push_back(s);
    }
    return 1;
}

int qmm_internal_chain_flush(qmm_ctx * c) { return c->chain_on ? chain_launch(c) : QMM_OK; }

extern "C" {

int qmm_abi_version(void) { return 2; }

const char * qmm_last_error(void) { return last_error().c_str(); }

int qmm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

qmm_ctx * qmm_create(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) {
        fail(QMM_ENODEV, "qmm_create: no HIP device %d (count %d)", device, n);
        return nullptr;
    }
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, device) != hipSuccess) {
        fail(QMM_ENODEV, "qmm_create: hipGetDeviceProperties failed");
        return nullptr;
    }
    if (strncmp(p.gcnArchName, "gfx950", 6) != 0) {
        fail(QMM_ENODEV, "qmm_create: device %d is %s; this library is built for gfx950 only", device, p.gcnArchName);
        return nullptr;
    }
    qmm_ctx * c = new qmm_ctx;
    c->device = device;
    c->cus = p.multiProcessorCount;
    snprintf(c->name, sizeof(c->name), "%s", p.name);
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc((void **) &c->flag, 16) != hipSuccess || hipMemset(c->flag, 0, 16) != hipSuccess) {
        fail(QMM_EHIP, "qmm_create: stream/flag setup failed");
        delete c;
        return nullptr;
    }
    c->kcnt_n = 1 << 16;
    if (hipMalloc((void **) &c->kcnt, (size_t) c->kcnt_n * sizeof(int)) != hipSuccess || hipMemset(c->kcnt, 0, (size_t) c->kcnt_n * sizeof(int)) != hipSuccess) {
        fail(QMM_EHIP, "qmm_create: split-K counters");
        delete c;
        return nullptr;
    }
    c->chain = new std::vector<ChainStep>();
    if (hipMalloc((void **) &c->chain_sync, sizeof(ChainSync)) != hipSuccess || hipMemset(c->chain_sync, 0, sizeof(ChainSync)) != hipSuccess) {
        fail(QMM_EHIP, "qmm_create: chain state setup failed");
        delete c->chain;
        delete c;
        return nullptr;
    }
    for (int j = 0; j < n; ++j) {                                   // row split copies between devices: peer access, best effort
        int can = 0;
        if (j != device && hipDeviceCanAccessPeer(&can, device, j) == hipSuccess && can) {
            const hipError_t pe = hipDeviceEnablePeerAccess(j, 0);
            if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) (void) hipGetLastError();
        }
    }
    (void) hipGetLastError();
    // the environment switches (qmm_switches.h), read for every context
    const qmm_sw::values sw = qmm_sw::read();
    c->splitk         = sw[qmm_sw::SW_SPLITK];
    c->act_mode       = sw[qmm_sw::SW_ACT_MODE] ? QMM_ACT_X86 : QMM_ACT_REF;
    c->mv_kmix        = sw[qmm_sw::SW_MV_KMIX];
    c->wide           = sw[qmm_sw::SW_WIDE];
    c->r64            = sw[qmm_sw::SW_R64];
    c->r64s           = sw[qmm_sw::SW_R64S];
    c->prep_reg       = sw[qmm_sw::SW_PREP_REG];
    c->regb_q23       = sw[qmm_sw::SW_REGB_Q23] != 0;
    c->mv_onepass     = sw[qmm_sw::SW_MV_ONEPASS];
    c->splitk_combine = sw[qmm_sw::SW_SPLITK_COMBINE];
    c->chain_enabled  = sw.is_set(qmm_sw::SW_CHAIN) ? sw[qmm_sw::SW_CHAIN] : 1;      // (the table's default is the plugin's: no chains unless asked)
    c->mv_bpc         = sw[qmm_sw::SW_MV_BPC];
    c->mm_group       = sw[qmm_sw::SW_MM_GROUP];
    c->skinny         = sw[qmm_sw::SW_SKINNY];
    if (sw[qmm_sw::SW_SKINNY_MAXN]) c->skinny_max_n = c->skinny_max_n_few = sw[qmm_sw::SW_SKINNY_MAXN];
    if (sw.is_set(qmm_sw::SW_ABLATE)) { int v = sw[qmm_sw::SW_ABLATE]; (void) hipMemcpyToSymbol(HIP_SYMBOL(g_mfma_dbg), &v, sizeof(int)); }
    c->prec           = qmm_sw::prec_is_bf16(sw.str(qmm_sw::SW_PREC)) ? QMM_PREC_BF16 : qmm_sw::prec_is_q8(sw.str(qmm_sw::SW_PREC)) ? QMM_PREC_Q8_EXACT : QMM_PREC_F16_Q8;
    return c;
}

void qmm_destroy(qmm_ctx * c) {
    if (!c) return;
    (void) hipSetDevice(c->device);
    (void) hipDeviceSynchronize();
    if (c->ws) (void) hipFree(c->ws);
    if (c->flag) (void) hipFree(c->flag);
    if (c->kcnt) (void) hipFree(c->kcnt);
    if (c->chain_sync) (void) hipFree(c->chain_sync);
    delete c->chain;
    delete c->trace;
    if (c->stream) (void) hipStreamDestroy(c->stream);
    delete c;
}

int qmm_device(const qmm_ctx * c) { return c ? c->device : -1; }

void * qmm_stream(const qmm_ctx * c) { return c ? (void *) c->stream : nullptr; }

int qmm_device_info(const qmm_ctx * c, char * name, size_t name_len, size_t * mem_free, size_t * mem_total, int * cus) {
    if (!c) return fail(QMM_EINVAL, "null ctx");
    HIP_TRY(hipSetDevice(c->device));
    if (name && name_len) snprintf(name, name_len, "%s", c->name);
    size_t f = 0, t = 0;
    HIP_TRY(hipMemGetInfo(&f, &t));
    if (mem_free) *mem_free = f;
    if (mem_total) *mem_total = t;
    if (cus) *cus = c->cus;
    return QMM_OK;
}

int qmm_set_act_mode(qmm_ctx * c, int m) {
    if (!c || (m != QMM_ACT_REF && m != QMM_ACT_X86)) return fail(QMM_EINVAL, "bad act mode");
    c->act_mode = m;
    return QMM_OK;
}
int qmm_set_precision(qmm_ctx * c, int p) {
    if (!c || (p != QMM_PREC_BF16 && p != QMM_PREC_F16_Q8 && p != QMM_PREC_Q8_EXACT)) return fail(QMM_EINVAL, "bad precision");
    c->prec = p;
    return QMM_OK;
}
int qmm_q8_exact_supported(int type, int64_t K) { return q8x_supports(type, K) ? 1 : 0; }

void * qmm_malloc(qmm_ctx * c, size_t bytes) {
    if (!c) return nullptr;
    void * p = nullptr;
    if (hipSetDevice(c->device) != hipSuccess || hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) {
        fail(QMM_ENOMEM, "hipMalloc(%zu) failed", bytes);
        return nullptr;
    }
    return p;
}
void qmm_free(qmm_ctx * c, void * p) {
    if (!c || !p) return;
    (void) hipSetDevice(c->device);
    (void) hipFree(p);
}
// page-locked host memory: transfers from / to it are real DMA and the *_async copies do not stage (the reference's
// counterpart is the rpcmem / ION pool shared with the cDSP, ggml-hexagon.cpp:4698-4747)
void * qmm_host_malloc(qmm_ctx * c, size_t bytes) {
    if (!c) return nullptr;
    void * p = nullptr;
    if (hipSetDevice(c->device) != hipSuccess || hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
        (void) hipGetLastError();
        fail(QMM_ENOMEM, "hipHostMalloc(%zu) failed", bytes);
        return nullptr;
    }
    return p;
}
void qmm_host_free(qmm_ctx * c, void * p) {
    if (!c || !p) return;
    (void) hipSetDevice(c->device);
    (void) hipHostFree(p);
}
int qmm_memcpy_h2d(qmm_ctx * c, void * dst, const void * src, size_t n, void * st) {
    HIP_TRY(hipSetDevice(c->device));
    QMM_CHAIN_FLUSH(c);
    HIP_TRY(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, c->s(st)));
    HIP_TRY(hipStreamSynchronize(c->s(st)));
    return QMM_OK;
}
int qmm_memcpy_d2h(qmm_ctx * c, void * dst, const void * src, size_t n, void * st) {
    HIP_TRY(hipSetDevice(c->device));
    QMM_CHAIN_FLUSH(c);
    HIP_TRY(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, c->s(st)));
    HIP_TRY(hipStreamSynchronize(c->s(st)));
    return QMM_OK;
}
int qmm_memcpy_d2d(qmm_ctx * c, void * dst, const void * src, size_t n, void * st) {
    HIP_TRY(hipSetDevice(c->device));
    QMM_CHAIN_FLUSH(c);
    HIP_TRY(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, c->s(st)));
    return QMM_OK;
}
struct qmm_event { hipEvent_t ev; };
int qmm_memcpy_h2d_async(qmm_ctx * c, void * dst, const void * src, size_t n, void * st) {
    if (!c) return fail(QMM_EINVAL, "null ctx");
    HIP_TRY(hipSetDevice(c->device));
    QMM_CHAIN_FLUSH(c);
    HIP_TRY(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, c->s(st)));
    return QMM_OK;
}
int qmm_memcpy_d2h_async(qmm_ctx * c, void * dst, const void * src, size_t n, void * st) {
    if (!c) return fail(QMM_EINVAL, "null ctx");
    HIP_TRY(hipSetDevice(c->device));
    QMM_CHAIN_FLUSH(c);
    HIP_TRY(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, c->s(st)));
    return QMM_OK;
}
int qmm_event_synchronize(qmm_ctx * c, qmm_event * e) {
    if (!c || !e) return fail(QMM_EINVAL, "qmm_event_synchronize: null argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(e->ev));
    return QMM_OK;
}
int qmm_memcpy2d_d2d(qmm_ctx * c, void * dst, size_t dpitch, const void * src, size_t spitch, size_t width, size_t height, void * st) {
    if (!c) return fail(QMM_EINVAL, "null ctx");
    if (width == 0 || height == 0) return QMM_OK;
    HIP_TRY(hipSetDevice(c->device));
    QMM_CHAIN_FLUSH(c);
    if (dpitch == width && spitch == width) HIP_TRY(hipMemcpyAsync(dst, src, width * height, hipMemcpyDeviceToDevice, c->s(st)));
    else HIP_TRY(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyDeviceToDevice, c->s(st)));
    return QMM_OK;
}
qmm_event * qmm_event_create(qmm_ctx * c) {
    if (!c || hipSetDevice(c->device) != hipSuccess) { fail(QMM_EINVAL, "qmm_event_create: bad ctx"); return nullptr; }
    qmm_event * e = new qmm_event;
    if (hipEventCreateWithFlags(&e->ev, hipEventDisableTiming) != hipSuccess) {
        fail(QMM_EHIP, "qmm_event_create: hipEventCreate failed");
        delete e;
        return nullptr;
    }
    return e;
}
qmm_event * qmm_event_create_timing(qmm_ctx * c) {
    if (!c || hipSetDevice(c->device) != hipSuccess) { fail(QMM_EINVAL, "qmm_event_create_timing: bad ctx"); return nullptr; }
    qmm_event * e = new qmm_event;
    if (hipEventCreate(&e->ev) != hipSuccess) {
        fail(QMM_EHIP, "qmm_event_create_timing: hipEventCreate failed");
        delete e;
        return nullptr;
    }
    return e;
}
int qmm_event_elapsed_ms(qmm_ctx * c, qmm_event * e0, qmm_event * e1, float * ms) {
    if (!c || !e0 || !e1 || !ms) return fail(QMM_EINVAL, "qmm_event_elapsed_ms: null argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventElapsedTime(ms, e0->ev, e1->ev));
    return QMM_OK;
}
void qmm_event_destroy(qmm_ctx * c, qmm_event * e) {
    if (!e) return;
    if (c) (void) hipSetDevice(c->device);
    (void) hipEventDestroy(e->ev);
    delete e;
}
int qmm_event_record(qmm_ctx * c, qmm_event * e, void * st) {
    if (!c || !e) return fail(QMM_EINVAL, "qmm_event_record: null argument");
    HIP_TRY(hipSetDevice(c->device));
    QMM_CHAIN_FLUSH(c);
    HIP_TRY(hipEventRecord(e->ev, c->s(st)));
    return QMM_OK;
}
int qmm_stream_wait_event(qmm_ctx * c, void * st, qmm_event * e) {
    if (!c || !e) return fail(QMM_EINVAL, "qmm_stream_wait_event: null argument");
    HIP_TRY(hipSetDevice(c->device));
    QMM_CHAIN_FLUSH(c);
    HIP_TRY(hipStreamWaitEvent(c->s(st), e->ev, 0));
    return QMM_OK;
}
int qmm_memset(qmm_ctx * c, void * dst, int v, size_t n, void * st) {
    HIP_TRY(hipSetDevice(c->device));
    QMM_CHAIN_FLUSH(c);
    HIP_TRY(hipMemsetAsync(dst, v, n, c->s(st)));
    return QMM_OK;
}
int qmm_synchronize(qmm_ctx * c, void * st) {
    HIP_TRY(hipSetDevice(c->device));
    if (c->chain_on && !c->chain->empty()) { int rc = chain_launch(c); if (rc) return rc; }       // nothing recorded stays behind a wait
    HIP_TRY(hipStreamSynchronize(c->s(st)));
    if (c->chain_launches != c->chain_checked) {
        uint32_t err = 0;
        HIP_TRY(hipMemcpy(&err, &c->chain_sync->err[0], sizeof(err), hipMemcpyDeviceToHost));
        c->chain_checked = c->chain_launches;
        if (err) {
            HIP_TRY(hipDeviceSynchronize());
            HIP_TRY(hipMemset(c->chain_sync, 0, sizeof(ChainSync)));
            return fail(QMM_EHIP, "chain: a grid-wide wait timed out (workgroups not co-resident?); results of that launch are undefined");
        }
    }
    if (c->mfma_calls != c->mfma_checked) {                  // prefill launches since the last look: did the f16 mode overflow?
        c->mfma_checked = c->mfma_calls;
        int nf = 0;
        HIP_TRY(hipMemcpyFromSymbol(&nf, HIP_SYMBOL(g_mfma_nonfinite), sizeof(int)));
        if (nf) {
            const int zero = 0;
            HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_mfma_nonfinite), &zero, sizeof(int)));
            return fail(QMM_EUNSUPPORTED, "prefill (f16 on Q8 activations) produced non-finite values: a weight block exceeds the f16 range (|w| >= 65504) "
                                          "or the activations are not finite; use QMM_PREC_BF16 (" QMM_SWITCH_ENV(PREC) "=bf16) for this model");
        }
    }
    if (c->id_calls != c->id_checked) {                      // MUL_MAT_ID launches since the last look: did a kernel meet an expert id out of range?
        c->id_checked = c->id_calls;
        int flag = 0;
        HIP_TRY(hipMemcpy(&flag, c->flag, sizeof(int), hipMemcpyDeviceToHost));
        if (flag) {
            HIP_TRY(hipMemset(c->flag, 0, sizeof(int)));
            return fail(QMM_EINVAL, "MUL_MAT_ID: expert id out of range seen by the kernel");
        }
    }
    return QMM_OK;
}

size_t qmm_row_size(int type, int64_t k) {
    if (type == T_BF16) return bf16_row_size(k);
    if (!type_known(type) || k % type_blck(type)) return 0;
    return (size_t) (k / type_blck(type)) * type_tsize(type);
}

// ------------------------------------------------------------------------------------------- codebooks

int qmm_set_codebook(qmm_ctx * c, int type, const uint32_t * entries, int n_entries) {
    if (!c || !entries) return fail(QMM_EINVAL, "qmm_set_codebook: NULL context or table");
    if (!type_codebook(type))
        return fail(QMM_EINVAL, "qmm_set_codebook: type %d takes no codebook (IQ2_XS = %d, IQ3_XXS = %d, IQ1_S = %d, IQ3_S = %d, IQ2_S = %d, IQ1_M = %d do)", type, T_IQ2_XS, T_IQ3_XXS, T_IQ1_S, T_IQ3_S, T_IQ2_S, T_IQ1_M);
    // (n_entries counts 32-bit words: an IQ2 or IQ1 entry of eight values is two of them)
    if (n_entries != type_codebook(type)) return fail(QMM_EINVAL, "qmm_set_codebook: type %d has %d entries, not %d", type, type_codebook(type), n_entries);
    // the units hold a magnitude with its sign as an int8 (neg4, qmm_device.hiph); IQ1's one table holds the int8 values themselves
    for (int i = 0; i < n_entries; ++i)
        for (int j = 0; j < 4; ++j) {
            const uint32_t v = (entries[i] >> (8 * j)) & 0xffu;
            if (type_ternary(type)) {
                if (v != 0xffu && v > 1) return fail(QMM_EUNSUPPORTED, "qmm_set_codebook: entry %d holds the byte 0x%02x; the IQ1 grid is -1, 0, +1 (0xff, 0x00, 0x01)", i / 2, v);
            } else if (v < 1 || v > 127) return fail(QMM_EUNSUPPORTED, "qmm_set_codebook: entry %d holds %u; the kernels take magnitudes in 1 .. 127", i, v);
        }
    HIP_TRY(hipSetDevice(c->device));
    QMM_CHAIN_FLUSH(c);
    HIP_TRY(hipDeviceSynchronize());                             // no launch in flight reads a table while it changes
    HIP_TRY(codebook_upload(type, entries, n_entries));
    if (const int rc = qmm_internal_ops_codebook(type, entries, n_entries)) return rc;
    if (const int rc = qmm_internal_matvec_codebook(type, entries, n_entries)) return rc;
    c->codebook[codebook_slot(type)] = true;
    return QMM_OK;
}

// ------------------------------------------------------------------------------------------- dequantize

int qmm_dequantize(qmm_ctx * c, int type, const void * w, int64_t rb, int64_t rows, int64_t K, float * dst, void * st) {
    if (c && type == T_BF16) {                                   // the exact f32 widening (qmm_bf16.hiph)
        const char * why = bf16_weight_refusal(w, rb, K, rows, rows);
        if (why || (uintptr_t) dst % 16) return fail(QMM_EINVAL, "qmm_dequantize: %s", why ? why : "dst must be 16-byte aligned");
        HIP_TRY(hipSetDevice(c->device));
        QMM_CHAIN_FLUSH(c);
        return run_bf16_widen(c->s(st), w, rb, rows, K, dst);
    }
    if (!c || !type_known(type)) return fail(QMM_EINVAL, "qmm_dequantize: bad ctx/type %d", type);
    if (const int rc = need_codebook(c, type, "qmm_dequantize")) return rc;
    if (K <= 0 || K % type_blck(type)) return fail(QMM_EINVAL, "qmm_dequantize: K=%lld", (long long) K);
    if (rb < (int64_t) qmm_row_size(type, K)) return fail(QMM_EINVAL, "qmm_dequantize: row stride too small");
    if (iq1m_misaligned(type, w, rb)) return fail(QMM_EINVAL, "qmm_dequantize: IQ1_M rows must be 8-byte aligned (base address and row stride multiples of 8)");
    if ((uintptr_t) dst % 16) return fail(QMM_EINVAL, "qmm_dequantize: dst must be 16-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    QMM_CHAIN_FLUSH(c);
    hipStream_t s = c->s(st);
#define QMM_X(TT) return launch_dequant<TT>(s, w, rb, rows, K, dst)
    QMM_FOR_TYPE(type, QMM_X)
#undef QMM_X
}

// ------------------------------------------------------------------------------------------- planar rows

int qmm_planar_type(int type, int64_t K, int64_t w_row_bytes) {
    if (type != T_Q4_0 && type != T_Q8_0 && type != T_Q6_K) return 0;
    if (K <= 0 || K % (type == T_Q6_K ? 2048 : 256) || w_row_bytes % 16) return 0;     // planes and rows start on 16-byte boundaries
    return type + 100;
}

int qmm_repack_rows(qmm_ctx * c, int type, void * w, int64_t w_row_bytes, int64_t rows, int64_t K, int to_planar, void * st) {
    if (!c) return fail(QMM_EINVAL, "qmm_repack_rows: NULL context");
    if (!qmm_planar_type(type, K, w_row_bytes) || (uintptr_t) w % 16 || w_row_bytes < (int64_t) qmm_row_size(type, K))
        return fail(QMM_EUNSUPPORTED, "qmm_repack_rows: type %d, K=%lld, row stride %lld has no planar form", type, (long long) K, (long long) w_row_bytes);
    if (rows <= 0) return QMM_OK;
    HIP_TRY(hipSetDevice(c->device));
    QMM_CHAIN_FLUSH(c);
    const size_t lds = qmm_row_size(type, K);
    if (lds > MV_LDS_FIT) return fail(QMM_EUNSUPPORTED, "qmm_repack_rows: a row of %zu bytes does not fit LDS", lds);
#define QMM_RP(TT, DIR)                                                                                                             \
    do {                                                                                                                            \
        auto kern = repack_rows_kernel<TT, DIR>;                                                                                    \
        if (lds > 64 * 1024) HIP_TRY(hipFuncSetAttribute((const void *) kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds)); \
        hipLaunchKernelGGL(kern, dim3((unsigned) rows), dim3(256), lds, c->s(st), (uint8_t *) w, w_row_bytes, (int) K);              \
    } while (0)
    if (type == T_Q4_0)      { if (to_planar) QMM_RP(T_Q4_0, true); else QMM_RP(T_Q4_0, false); }
    else if (type == T_Q8_0) { if (to_planar) QMM_RP(T_Q8_0, true); else QMM_RP(T_Q8_0, false); }
    else                     { if (to_planar) QMM_RP(T_Q6_K, true); else QMM_RP(T_Q6_K, false); }
#undef QMM_RP
    HIP_TRY(hipGetLastError());
    return QMM_OK;
}

// ------------------------------------------------------------------------------------------- quantize_act

int qmm_quantize_act(qmm_ctx * c, int vt, const float * x, int64_t rows, int64_t K, int64_t ldx,
                     int8_t * q, float * d, int16_t * bs, void * st) {
    if (!c || (vt != T_Q8_0 && vt != T_Q8_1 && vt != T_Q8_K)) return fail(QMM_EINVAL, "qmm_quantize_act: vec_dot_type %d", vt);
    if (vt == T_Q8_1 && (!bs || (uintptr_t) bs % 4)) return fail(QMM_EINVAL, "qmm_quantize_act: Q8_1 wants the s array (f32 [rows, K/32]) in `bs`");
    if (K <= 0 || K % (vt == T_Q8_K ? 256 : 32) || ldx % 4 || (uintptr_t) x % 16 || (uintptr_t) q % 4)
        return fail(QMM_EINVAL, "qmm_quantize_act: K/ldx/alignment");
    if (rows == 0) return QMM_OK;
    HIP_TRY(hipSetDevice(c->device));
    QMM_CHAIN_FLUSH(c);
    const int rpb = 4;
    dim3 grid((unsigned) ((rows + rpb - 1) / rpb));
    if (vt == T_Q8_0)
        hipLaunchKernelGGL((quantize_act_kernel<T_Q8_0>), grid, dim3(256), 0, c->s(st), x, ldx, (int) rows, (int) K, c->act_mode, q, d, bs, rpb);
    else if (vt == T_Q8_1)
        hipLaunchKernelGGL((quantize_act_kernel<T_Q8_1>), grid, dim3(256), 0, c->s(st), x, ldx, (int) rows, (int) K, c->act_mode, q, d, bs, rpb);
    else
        hipLaunchKernelGGL((quantize_act_kernel<T_Q8_K>), grid, dim3(256), 0, c->s(st), x, ldx, (int) rows, (int) K, c->act_mode, q, d, bs, rpb);
    HIP_TRY(hipGetLastError());
    return QMM_OK;
}

// ------------------------------------------------------------------------------------------- mat-vec

// `ex`: what the few-token kernels fold in (N <= QMM_MATVEC_MAX_N); `in`: what the activation prep of a prompt batch forms (above)
static int mul_mat_group_impl(qmm_ctx * c, const qmm_weight * ws, int nw, int64_t K, const float * x, int64_t N, int64_t ldx, void * stream,
                              const qmm_mv_extra * ex, const PrefillInput & in = PrefillInput{}) {
    if (!c || !ws || nw <= 0) return fail(QMM_EINVAL, "qmm_mul_mat_group: bad arguments");
    if (N <= 0) return QMM_OK;
    int n_bf16 = 0;
    for (int i = 0; i < nw; ++i) n_bf16 += ws[i].type == T_BF16;
    if (n_bf16) {
        // BF16 matrices go to their own plan (qmm_bf16_plan.h) before the quantized machinery sees them: no fold, no chain step, no
        // precision or activation mode.  A group that mixes them with other types runs as consecutive launches, one per same-kind run.
        const bool folds = in.flags() || (ex && (ex->norm_w || ex->swiglu || ex->norm_add || ex->residual[0] || ex->residual[1] || ex->residual[2] || ex->residual[3]));
        if (folds) return fail(QMM_EUNSUPPORTED, "qmm_mul_mat_group: BF16 matrices take no norm, residual or SwiGLU fold");
        if (n_bf16 < nw) {
            for (int first = 0, next; first < nw; first = next) {
                for (next = first + 1; next < nw && (ws[next].type == T_BF16) == (ws[first].type == T_BF16); ++next) {}
                const int rc = mul_mat_group_impl(c, ws + first, next - first, K, x, N, ldx, stream, nullptr);
                if (rc) return rc;
            }
            return QMM_OK;
        }
        const int rc = bf16_check(ws, nw, K, x, N, ldx);
        if (rc) return rc;
        HIP_TRY(hipSetDevice(c->device));
        QMM_CHAIN_FLUSH(c);                                      // inside a recording: what was collected first, then this, directly
        return run_bf16(c, c->s(stream), ws, nw, K, x, N, ldx);
    }
    if (ex) {                                                    // few-token extras: validated by the plan header, whatever N
        char msg[160];
        const int rc = matvec_extras_check(ws, nw, K, N, ex, msg, sizeof(msg));
        if (rc) return fail(rc, "%s", msg);
    }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->s(stream);
    for (int i = 0; i < nw; ++i) {
        int rc = check_mm(c, ws[i].type, ws[i].w, ws[i].w_row_bytes, K, x, ldx, "qmm_mul_mat");
        if (rc) return rc;
        if (ws[i].M < 0 || ws[i].ldd < ws[i].M) return fail(QMM_EINVAL, "qmm_mul_mat: ldd < M");
    }
    if (c->chain_on) {
        // recording (qmm_chain_begin): one-token groups are collected; anything else goes out behind what was collected
        int rec = N == 1 ? chain_record(c, st, ws, nw, K, x, ldx, ex) : 0;
        if (rec < 0) return rec;
        if (rec == 1) return QMM_OK;
        int rc = chain_launch(c);
        if (rc) return rc;
    }
    if (N <= QMM_MATVEC_MAX_N) {
        // few tokens: the plan (qmm_matvec_plan.h) lists the launches, run by run of the group's matrices; this executes it
        const MatvecRules rules = matvec_rules(c);
        for (int first = 0; first < nw;) {
            const MatvecPlan plan = matvec_group_plan(rules, ws, nw, K, N, ex, first);
            for (int k = 0; k < plan.n; ++k) {
                const MatvecLaunch & l = plan.launch[k];
                int rc = run_matvec(c, st, l, matvec_group(ws, l.idx, l.row_end, l.n, l.n0, ex), x + l.n0 * ldx, ldx);
                if (rc) return rc;
            }
            first = plan.next;
        }
        return QMM_OK;
    }
    // a prompt batch: the group shares src1, whose 16-bit operand is prepared once per activation format (key); the group's plan
    // (qmm_prefill_plan.h) lists the launches, run_prefill_group (qmm_prefill.hiph) issues them
    c->mfma_calls++;
    return run_prefill_group(c, st, ws, nw, K, x, N, ldx, in);
}

// dst = W * (silu(gate) .* up) for a prompt batch: ffn_down with the SwiGLU product formed by the activation prep of the MFMA path
// (one workgroup per token row reads both rows), so the product never exists in HBM.  Few-token batches fold it on the
// producer side instead (qmm_mv_extra.swiglu).
int qmm_mul_mat_swiglu_in(qmm_ctx * c, int type, const void * w, int64_t w_row_bytes, int64_t K, int64_t M, const float * gate, int64_t ld_gate,
                          const float * up, int64_t ld_up, int64_t N, float * dst, int64_t ldd, void * stream) {
    if (!c) return fail(QMM_EINVAL, "qmm_mul_mat_swiglu_in: NULL context");
    if (N <= QMM_MATVEC_MAX_N) return fail(QMM_EUNSUPPORTED, "qmm_mul_mat_swiglu_in: batches above %d tokens (below: qmm_mv_extra.swiglu)", QMM_MATVEC_MAX_N);
    if (c->prec != QMM_PREC_F16_Q8) return fail(QMM_EUNSUPPORTED, "qmm_mul_mat_swiglu_in: only in the default prefill mode");
    if ((uintptr_t) up % 16 || ld_up % 4 || ld_up < K) return fail(QMM_EINVAL, "qmm_mul_mat_swiglu_in: up must be 16-byte aligned, ld_up %% 4 == 0, ld_up >= K");
    const qmm_weight ws = { w, w_row_bytes, M, dst, ldd, type };
    PrefillInput in;
    in.x2 = up;  in.ldx2 = ld_up;
    return mul_mat_group_impl(c, &ws, 1, K, gate, N, ld_gate, stream, nullptr, in);
}

int qmm_mul_mat_group(qmm_ctx * c, const qmm_weight * ws, int nw, int64_t K, const float * x, int64_t N, int64_t ldx, void * stream) {
    return mul_mat_group_impl(c, ws, nw, K, x, N, ldx, stream, nullptr);
}

int qmm_mul_mat_group_norm_supported(qmm_ctx * c, const qmm_weight * ws, int nw, int64_t K, int64_t N) {
    if (!c || !ws || nw < 1 || nw > MV_MAX_GROUP || N <= QMM_MATVEC_MAX_N || K <= 0 || K % 1024 || K > 16384) return 0;
    if (c->prec != QMM_PREC_F16_Q8 || !c->prep_reg) return 0;
    for (int i = 0; i < nw; ++i) {
        const int t = type_base(ws[i].type);
        if (!type_known(ws[i].type) || type_act(t) != T_Q8_K || t == T_IQ4_XS || !mfma_regb_supports(c, t)) return 0;
    }
    return 1;
}

int qmm_mul_mat_group_ex(qmm_ctx * c, const qmm_weight * ws, int nw, int64_t K, const float * x, int64_t N, int64_t ldx, const qmm_mv_extra * ex,
                         void * stream) {
    bool bf16 = false;
    for (int i = 0; ws && i < nw; ++i) bf16 = bf16 || ws[i].type == T_BF16;
    if (c && ex && N > QMM_MATVEC_MAX_N && !bf16) {
        // a prompt batch: only the norm in front of the group (the activation prep forms it); everything else is the few-token kernels'
        if (!ex->norm_w || ex->swiglu || ex->residual[0] || ex->residual[1] || ex->residual[2] || ex->residual[3])
            return fail(QMM_EUNSUPPORTED, "qmm_mul_mat_group_ex: batches of more than %d tokens take the norm only", QMM_MATVEC_MAX_N);
        if (!qmm_mul_mat_group_norm_supported(c, ws, nw, K, N)) return fail(QMM_EUNSUPPORTED, "qmm_mul_mat_group_ex: this group does not take a fused norm at %lld tokens", (long long) N);
        if (ex->norm_eps < 0.0f || (uintptr_t) ex->norm_w % 16 || (uintptr_t) x % 16 || ldx % 4 || (ex->norm_add && ((uintptr_t) ex->norm_add % 16 || ex->norm_add_ld % 4 || !ex->norm_sum)) ||
            (ex->norm_sum && ((uintptr_t) ex->norm_sum % 16 || ex->norm_sum_ld % 4)))
            return fail(QMM_EINVAL, "qmm_mul_mat_group_ex: norm operands must be 16-byte aligned rows, eps >= 0, a sum buffer with norm_add");
        PrefillInput in;
        in.norm = { ex->norm_w, ex->norm_eps, ex->norm_add, ex->norm_add_ld, ex->norm_add ? ex->norm_sum : nullptr, ex->norm_sum_ld };
        return mul_mat_group_impl(c, ws, nw, K, x, N, ldx, stream, nullptr, in);
    }
    return mul_mat_group_impl(c, ws, nw, K, x, N, ldx, stream, ex);
}

int qmm_mul_mat(qmm_ctx * c, int type, const void * w, int64_t rb, int64_t K, int64_t M,
                const float * x, int64_t N, int64_t ldx, float * dst, int64_t ldd, void * stream) {
    qmm_weight ws = { w, rb, M, dst, ldd, type };
    return qmm_mul_mat_group(c, &ws, 1, K, x, N, ldx, stream);
}

// what the MUL_MAT_ID entry points check alike (who: the entry point, for the messages; second: its second tensor and destination are there)
static int check_mm_id(const qmm_ctx * c, const char * who, bool second, int type, const void * as, int64_t rb, int64_t expert_bytes, int64_t K, const float * b, int64_t ne11,
                       int64_t b_nb1, int64_t b_nb2, int64_t ids_nb1, int64_t n_used, int64_t d_nb1, int64_t d_nb2) {
    if (!c) return fail(QMM_EINVAL, "null ctx");
    if (!second) return fail(QMM_EINVAL, "%s: second tensor missing", who);
    const int rc = check_mm(c, type, as, rb, K, b, K, who);
    if (rc) return rc;
    if (b_nb1 % 16 || b_nb2 % 16 || ids_nb1 % 4 || d_nb1 % 4 || d_nb2 % 4 || expert_bytes % 2 || (ne11 != 1 && ne11 != n_used)) return fail(QMM_EINVAL, "%s: strides / ne11", who);
    if (iq1m_misaligned(type, as, rb, expert_bytes)) return fail(QMM_EINVAL, "%s: IQ1_M experts must be 8-byte aligned (expert stride a multiple of 8)", who);
    return QMM_OK;
}

int qmm_mul_mat_id(qmm_ctx * c, int type, const void * as, int64_t rb, int64_t expert_bytes,
                   int64_t K, int64_t M, int64_t n_expert,
                   const float * b, int64_t ne11, int64_t b_nb1, int64_t b_nb2,
                   const int32_t * ids, int64_t n_used, int64_t n_tokens, int64_t ids_nb1,
                   float * dst, int64_t d_nb1, int64_t d_nb2, void * stream) {
    const int rc = check_mm_id(c, "qmm_mul_mat_id", true, type, as, rb, expert_bytes, K, b, ne11, b_nb1, b_nb2, ids_nb1, n_used, d_nb1, d_nb2);
    if (rc) return rc;
    if (n_tokens <= 0 || n_used <= 0 || M <= 0) return QMM_OK;
    HIP_TRY(hipSetDevice(c->device));
    QMM_CHAIN_FLUSH(c);
    c->mfma_calls++;
    c->id_calls++;
    return moe_mul_mat_id(c, c->s(stream), type, as, rb, expert_bytes, K, M, n_expert, b, ne11, b_nb1, b_nb2,
                          ids, n_used, n_tokens, ids_nb1, dst, d_nb1, d_nb2);
}

int qmm_mul_mat_id_pair(qmm_ctx * c, int type, const void * as0, const void * as1, int64_t rb, int64_t expert_bytes,
                        int64_t K, int64_t M, int64_t n_expert,
                        const float * b, int64_t ne11, int64_t b_nb1, int64_t b_nb2,
                        const int32_t * ids, int64_t n_used, int64_t n_tokens, int64_t ids_nb1,
                        float * dst0, float * dst1, int64_t d_nb1, int64_t d_nb2, void * stream) {
    const int rc = check_mm_id(c, "qmm_mul_mat_id_pair", as1 && dst1, type, as0, rb, expert_bytes, K, b, ne11, b_nb1, b_nb2, ids_nb1, n_used, d_nb1, d_nb2);
    if (rc) return rc;
    if (n_tokens <= 0 || n_used <= 0 || M <= 0) return QMM_OK;
    HIP_TRY(hipSetDevice(c->device));
    QMM_CHAIN_FLUSH(c);
    c->mfma_calls++;
    c->id_calls++;
    return moe_mul_mat_id(c, c->s(stream), type, as0, rb, expert_bytes, K, M, n_expert, b, ne11, b_nb1, b_nb2,
                          ids, n_used, n_tokens, ids_nb1, dst0, d_nb1, d_nb2, as1, dst1);
}

int qmm_mul_mat_id_swiglu_supported(int64_t n_used, int64_t n_tokens) {
    return moe_runs_as_matvec(n_used, n_tokens);
}

int qmm_mul_mat_id_swiglu(qmm_ctx * c, int type, const void * as_gate, const void * as_up, int64_t rb, int64_t expert_bytes,
                          int64_t K, int64_t M, int64_t n_expert,
                          const float * b, int64_t ne11, int64_t b_nb1, int64_t b_nb2,
                          const int32_t * ids, int64_t n_used, int64_t n_tokens, int64_t ids_nb1,
                          float * dst, int64_t d_nb1, int64_t d_nb2, void * stream) {
    const int rc = check_mm_id(c, "qmm_mul_mat_id_swiglu", as_up && dst, type, as_gate, rb, expert_bytes, K, b, ne11, b_nb1, b_nb2, ids_nb1, n_used, d_nb1, d_nb2);
    if (rc) return rc;
    if (!qmm_mul_mat_id_swiglu_supported(n_used, n_tokens)) return fail(QMM_EUNSUPPORTED, "qmm_mul_mat_id_swiglu: more than %d (token, slot) pairs", MOE_MATVEC_MAX_PAIRS);
    if (M <= 0) return QMM_OK;
    HIP_TRY(hipSetDevice(c->device));
    QMM_CHAIN_FLUSH(c);
    c->id_calls++;
    return moe_mul_mat_id(c, c->s(stream), type, as_gate, rb, expert_bytes, K, M, n_expert, b, ne11, b_nb1, b_nb2, ids, n_used, n_tokens, ids_nb1, dst, d_nb1, d_nb2, as_up, nullptr, MOE_MV_SWIGLU);
}

int qmm_chain_begin(qmm_ctx * c) {
    if (!c) return fail(QMM_EINVAL, "qmm_chain_begin: NULL context");
    if (c->chain_on) return fail(QMM_EINVAL, "qmm_chain_begin: already recording");
    c->chain_on = c->chain_enabled != 0;
    return QMM_OK;
}
int qmm_chain_flush(qmm_ctx * c) {
    if (!c) return fail(QMM_EINVAL, "qmm_chain_flush: NULL context");
    if (!c->chain_on) return QMM_OK;
    HIP_TRY(hipSetDevice(c->device));
    return chain_launch(c);
}
int qmm_chain_end(qmm_ctx * c) {
    if (!c) return fail(QMM_EINVAL, "qmm_chain_end: NULL context");
    int rc = QMM_OK;
    if (c->chain_on) {
        HIP_TRY(hipSetDevice(c->device));
        rc = chain_launch(c);
    }
    c->chain_on = false;
    return rc;
}
int qmm_chain_debug(qmm_ctx * c, void * stamps) {
    if (!c) return fail(QMM_EINVAL, "qmm_chain_debug: NULL context");
    c->chain_dbg = (uint64_t *) stamps;
    return QMM_OK;
}
int qmm_trace_begin(qmm_ctx * c) {
    if (!c) return fail(QMM_EINVAL, "qmm_trace_begin: NULL context");
    if (!c->trace) c->trace = new std::string();
    c->trace->clear();
    return QMM_OK;
}

int qmm_trace_end(qmm_ctx * c, char * buf, size_t len) {
    if (!c || !c->trace) return fail(QMM_EINVAL, "qmm_trace_end: no trace in progress");
    int n = 0;
    for (char ch : *c->trace) n += ch == ';';
    if (buf && len) {
        snprintf(buf, len, "%s", c->trace->c_str());
        if (c->trace->size() >= len) n = fail(QMM_EINVAL, "qmm_trace_end: %zu bytes of labels do not fit the buffer", c->trace->size());
    }
    delete c->trace;
    c->trace = nullptr;
    return n;
}

int qmm_chain_stats(const qmm_ctx * c, int * launches, int * steps) {
    if (!c) return fail(QMM_EINVAL, "qmm_chain_stats: NULL context");
    if (launches) *launches = c->chain_launches;
    if (steps) *steps = c->chain_steps;
    return QMM_OK;
}

} // extern "C"
