// mv_dev.hip — development harness of the one-token mat-vec launch (csrc/qmm_matvec.hiph matvec_kernel<T, 1, false>): the llama3-8b
// token-generation launches that one kernel type serves, each on rotating weight sets larger than the Infinity Cache, grid / block /
// LDS bytes as the launch plan has them (csrc/qmm_matvec_plan.h).  Built with and without the workgroup barrier between the
// activation loads and the weight requests (MV_ACT_FIRST, qmm_matvec.hiph), with the row lookup behind the activation loads or at
// kernel entry (MV_HEAD_FIRST), with or without kernel-argument preload, timed and stamped.  The mixed-type q/k/v launch goes through
// matvec_kmix_kernel<1, false>.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize [-DMV_ACT_FIRST=0] [-DMV_HEAD_FIRST=0]
//         [-mllvm -amdgpu-kernarg-preload-count=8] -o mv_dev profiles/tools/mv_dev.hip && ./mv_dev
//       times the launches, replayed from a hipGraph: median and spread of 15 windows; prints a checksum of the outputs (the same in
//       every build: the barrier moves no bit)
//   hipcc ... -DMV_STAMPS -o mv_dev_stamps profiles/tools/mv_dev.hip && ./mv_dev_stamps
//       the 100 MHz phase stamps of wave 0 of every workgroup (never quote this build's times: read where the phases lie):
//       entry | first activation loads issued | activations and first slice requested | the wave's staging done | barrier passed | first slice dotted | last store
//       "first slice dotted" directly behind "barrier passed" says the slice had landed during the staging.
#include "../../ggml-hexagon_amd/csrc/qmm_matvec.hiph"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

using namespace qmm;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

using Kern = void (*)(const float *, int64_t, int, int, int, MatvecGroup);
struct Shape { const char * name; int type, K, n, M[MV_MAX_GROUP]; bool mixed; };   // mixed: the last matrix is planar Q6_K

int main() {
    setvbuf(stdout, nullptr, _IONBF, 0);
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    const Shape shapes[] = {
        { "down Q4_K 4096 x 14336",            T_Q4_K,  14336, 1, { 4096 } },
        { "down planar Q6_K 4096 x 14336",     T_Q6_KP, 14336, 1, { 4096 } },
        { "q/k/v Q4_K 4096+1024+1024 x 4096",  T_Q4_K,  4096,  3, { 4096, 1024, 1024 } },
        { "wo Q4_K 4096 x 4096",               T_Q4_K,  4096,  1, { 4096 } },
        { "gate+up Q4_K 2 x 14336 x 4096",     T_Q4_K,  4096,  2, { 14336, 14336 } },
        { "q/k/v mixed 4096+1024 Q4_K, 1024 planar Q6_K x 4096", T_Q4_K, 4096, 3, { 4096, 1024, 1024 }, true },
        { "output planar Q6_K 128256 x 4096",  T_Q6_KP, 4096,  1, { 128256 } },
    };
    std::mt19937 rng(7);
    hipStream_t st;
    CK(hipStreamCreate(&st));
    for (const Shape & s : shapes) {
        int64_t rbs[MV_MAX_GROUP];
        int types[MV_MAX_GROUP], row_end[MV_MAX_GROUP], rows = 0;
        size_t offs[MV_MAX_GROUP], bytes = 0;
        for (int i = 0; i < s.n; ++i) {
            types[i] = s.mixed && i == s.n - 1 ? T_Q6_KP : s.type;
            rbs[i] = (int64_t) s.K / 256 * (types[i] == T_Q4_K ? 144 : 210);
            row_end[i] = rows += s.M[i];
            offs[i] = bytes;
            bytes += (size_t) s.M[i] * rbs[i];
        }
        const int sets = (int) std::min<size_t>(48, ((size_t) 320 << 20) / bytes + 2);
        // every byte below 0x40: finite f16 scales whatever field a byte lands in (the values do not matter, their bits must agree)
        std::vector<uint8_t> hw(bytes);
        for (auto & b : hw) b = (uint8_t) (rng() & 0x3f);
        std::vector<float> hx(s.K);
        for (auto & v : hx) v = ((int) (rng() % 2001) - 1000) / 1000.0f;
        uint8_t * w; float * x, * dst;
        CK(hipMalloc(&w, bytes * sets)); CK(hipMalloc(&x, s.K * 4)); CK(hipMalloc(&dst, (size_t) rows * 4));
        for (int k = 0; k < sets; ++k) CK(hipMemcpy(w + bytes * k, hw.data(), bytes, hipMemcpyHostToDevice));
        CK(hipMemcpy(x, hx.data(), s.K * 4, hipMemcpyHostToDevice));
        const MatvecRules rules = { cus, 1, 2, 1, QMM_ACT_REF };
        const MatvecLaunch plan = matvec_launch(rules, s.mixed ? MV_MIXED : MV_PER_TYPE, s.type, nullptr, row_end, s.n, s.K, 0, 1, false, 0, nullptr);
        if (plan.error) { fprintf(stderr, "%s: refused\n", s.name); return 2; }
        const Kern kern = s.mixed ? matvec_kmix_kernel<1, false> : s.type == T_Q4_K ? matvec_kernel<T_Q4_K, 1, false> : matvec_kernel<T_Q6_KP, 1, false>;
        auto launch = [&](int set) {
            MatvecGroup g;
            memset(&g, 0, sizeof(g));
            for (int i = 0; i < s.n; ++i) {
                g.w[i] = w + bytes * set + offs[i];
                g.dst[i] = dst + (i ? row_end[i - 1] : 0);
                g.row_bytes[i] = rbs[i];  g.ldd[i] = s.M[i];  g.row_end[i] = row_end[i];  g.type[i] = types[i];
            }
            g.n = s.n;
            hipLaunchKernelGGL(kern, dim3(plan.blocks), dim3(plan.waves * WAVE), plan.lds, st, x, (int64_t) s.K, s.K, plan.act_arg, rows, g);
        };
        std::vector<float> o(rows);
        CK(hipMemsetAsync(dst, 0xff, (size_t) rows * 4, st));
        launch(0);
        CK(hipStreamSynchronize(st));
        CK(hipMemcpy(o.data(), dst, (size_t) rows * 4, hipMemcpyDeviceToHost));
        uint32_t sum = 0;
        for (float v : o) { uint32_t u; memcpy(&u, &v, 4); sum = sum * 31 + u; }
        printf("%-36s %5.1f MB x %2d sets, grid %d x %d, barrier %s, head %s, output bits %08x\n", s.name, bytes / 1e6, sets, plan.blocks, plan.waves * WAVE, MV_ACT_FIRST ? "on" : "off", MV_HEAD_FIRST ? "new" : "old", sum);
#ifdef MV_STAMPS
        static const char * names[7] = { "entry", "first act load", "requests out", "own staging done", "barrier passed", "first slice dotted", "last store" };
        static const int slot[7] = { 0, 6, 1, 2, 3, 4, 5 };
        if (!s.mixed) {                                                        // (matvec_kmix_kernel carries no stamps)
            for (int k = 0; k < sets; ++k) launch(k);                          // the stamped launch reads a set that has left the cache
            CK(hipStreamSynchronize(st));
            static unsigned long long stamps[512][8];
            CK(hipMemcpyFromSymbol(stamps, HIP_SYMBOL(mv_stamps), sizeof(stamps)));
            const int nb = std::min(plan.blocks, 512);
            unsigned long long t0 = ~0ull;
            for (int b = 0; b < nb; ++b) t0 = std::min(t0, stamps[b][0]);
            printf("  us from the first workgroup's entry, median / max over %d workgroups:", nb);
            for (int k = 0; k < 7; ++k) {
                std::vector<double> v;
                for (int b = 0; b < nb; ++b) v.push_back((double) (stamps[b][slot[k]] - t0) / 100.0);
                std::sort(v.begin(), v.end());
                printf("%s %s %.2f / %.2f", k ? " |" : "", names[k], v[nb / 2], v[nb - 1]);
            }
            printf("\n");
        }
#else
        const int reps = 25, windows = 15;
        hipGraph_t graph;
        hipGraphExec_t exec;
        CK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        for (int i = 0; i < reps * sets; ++i) launch(i % sets);
        CK(hipStreamEndCapture(st, &graph));
        CK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
        CK(hipGraphDestroy(graph));
        CK(hipGraphLaunch(exec, st));
        CK(hipStreamSynchronize(st));
        hipEvent_t e0, e1;
        CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
        std::vector<double> us;
        for (int wdw = 0; wdw < windows; ++wdw) {
            CK(hipEventRecord(e0, st));
            CK(hipGraphLaunch(exec, st));
            CK(hipEventRecord(e1, st));
            CK(hipEventSynchronize(e1));
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            us.push_back(ms * 1e3 / (reps * sets));
        }
        std::sort(us.begin(), us.end());
        printf("  %6.2f us per launch (median of %d windows, %.2f .. %.2f)\n", us[windows / 2], windows, us[0], us[windows - 1]);
        CK(hipGraphExecDestroy(exec));
        CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
#endif
        CK(hipFree(w)); CK(hipFree(x)); CK(hipFree(dst));
    }
    return 0;
}
