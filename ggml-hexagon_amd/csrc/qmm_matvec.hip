// qmm_matvec.hip — the instantiations of the few-token mat-vec kernels (qmm_matvec.hiph: matvec_kernel, matvec_kmix_kernel) as a
// translation unit of their own, because it is compiled with kernel-argument preload (-mllvm -amdgpu-kernarg-preload-count=8,
// ggml_hexagon_amd/build.py): x, ldx, K, act_mode and total_rows, the kernels' leading parameters, arrive in scalar registers, so the
// first activation load waits for no kernel-argument read.  The flag holds for a whole translation unit and moves
// the registers of every kernel in it; the prefill, MoE, chain and BF16 kernels stay in qmm_api.hip, compiled as they were.
// Host side: which instantiation a launch plan names, and this code object's copy of the codebook tables.

#include "qmm_host.h"

#include "qmm_matvec.hiph"

using namespace qmm;

static_assert(QMM_MATVEC_MAX_N == 8, "QMM_FOR_NTOK lists the token counts");

// the plan's instantiation for NT tokens (with Q8_0 matrices in a mixed group the kernel exists for NT <= 4 only, no fused norm: matvec_group_plan)
template <int NT> static MatvecKernel matvec_instance(const MatvecLaunch & l) {
    if constexpr (NT <= 4) {
        if (l.kind == MV_MIXED_Q80) return l.ex ? matvec_kmix_kernel<NT, true, true> : matvec_kmix_kernel<NT, false, true>;
    }
    if (l.kind != MV_PER_TYPE) return l.ex ? matvec_kmix_kernel<NT, true> : matvec_kmix_kernel<NT, false>;
#define QMM_X(TT) return l.ex ? matvec_kernel<TT, NT, true> : matvec_kernel<TT, NT, false>
    QMM_FOR_TYPE(l.type, QMM_X)
#undef QMM_X
    return nullptr;
}

MatvecKernel qmm_internal_matvec_kernel(const MatvecLaunch & l) {
    MatvecKernel kern = nullptr;
#define QMM_X(NT) kern = matvec_instance<NT>(l); break
    QMM_FOR_NTOK(l.ntok, QMM_X)
#undef QMM_X
    return kern;
}

// qmm_set_codebook (qmm_api.hip) writes every code object's tables: this one's serve the mat-vec kernels of the codebook types
int qmm_internal_matvec_codebook(int type, const uint32_t * entries, int n) {
    HIP_TRY(codebook_upload(type, entries, n));
    return QMM_OK;
}
