#!/usr/bin/env python3
"""writes tests/cpp/qmm_stub.cpp from the C-ABI headers: host memory behind the pointers, no compute (see the file's header).
With QMM_STUB_TRACE=<file> in the environment the stub appends one line per launch and per *_supported probe to that file: two builds
of the plugin that make the same calls in the same order with the same arguments write the same text."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
special = {
    "qmm_abi_version": "return 2;",
    "qmm_last_error": 'return "stub";',
    "qmm_device_count": "return 1;",
    "qmm_create": "return (qmm_ctx *) memset(stub_alloc(64), 0, 64);",
    "qmm_destroy": "stub_release(ctx);",
    "qmm_device": "return 0;",
    "qmm_stream": "return nullptr;",
    "qmm_device_info": 'if (name && name_len) snprintf(name, name_len, "stub"); if (mem_free) *mem_free = (size_t) 64 << 30; '
                       'if (mem_total) *mem_total = (size_t) 64 << 30; if (compute_units) *compute_units = 256; return 0;',
    "qmm_malloc": "return stub_alloc(bytes);",
    "qmm_free": "stub_release(dptr);",
    "qmm_host_malloc": "return aligned_alloc(256, (bytes + 256) & ~(size_t) 255);",
    "qmm_host_free": "free(hptr);",
    "qmm_memcpy_h2d": "memcpy(dst, src, bytes); return 0;",
    "qmm_memcpy_d2h": "memcpy(dst, src, bytes); return 0;",
    "qmm_memcpy_d2d": "memmove(dst, src, bytes); return 0;",
    "qmm_memcpy_h2d_async": "memcpy(dst, src, bytes); return 0;",
    "qmm_memcpy_d2h_async": "memcpy(dst, src, bytes); return 0;",
    "qmm_memset": "memset(dst, value, bytes); return 0;",
    "qmm_memcpy2d_d2d": "for (size_t r = 0; r < height; ++r) memmove((char *) dst + r * dpitch, (const char *) src + r * spitch, width); return 0;",
    "qmm_event_create": "return (qmm_event *) calloc(1, 8);",
    "qmm_event_create_timing": "return (qmm_event *) calloc(1, 8);",
    "qmm_event_destroy": "free(ev);",
    "qmm_event_elapsed_ms": "*ms = 0.0f; return 0;",
    "qmm_row_size": "static const int tsz[] = {0,0,18,20,0,0,22,24,34,36,84,110,144,176,210,292,0,0,0,0,18}; const int t = type >= 100 ? type - 100 : type; "
                    "if (t < 0 || t > 20 || !tsz[t]) return 0; const int b = (t >= 10 && t <= 15) ? 256 : 32; return k % b ? 0 : (size_t) (k / b) * tsz[t];",
    "qmm_planar_type": "if (type != 2 && type != 8 && type != 14) return 0; if (K <= 0 || K % (type == 14 ? 2048 : 256) || w_row_bytes % 16) return 0; return type + 100;",
    "qmm_comm_create": "return -5;",      # no RCCL behind the stub: the plugin must fall back to peer copies
    "qmm_chain_stats": "if (persistent_launches) *persistent_launches = 0; if (steps_in_them) *steps_in_them = 0; return 0;",
}
TRACE_SUPPORT = r"""namespace {
struct stub_block { const char * base; size_t bytes; long ord; };
std::vector<stub_block> g_blocks;                    // live qmm_malloc / qmm_create blocks, recorded only while tracing
long g_ord = 0;
std::mutex g_mu;
FILE * trace_file() {
    static FILE * f = [] { const char * p = getenv("QMM_STUB_TRACE"); return p && *p ? fopen(p, "a") : nullptr; }();
    return f;
}
void * stub_alloc(size_t bytes) {
    void * p = aligned_alloc(256, (bytes + 256) & ~(size_t) 255);       // aligned as device allocations are: the buffer code relies on it
    if (p && trace_file()) { std::lock_guard<std::mutex> lock(g_mu); g_blocks.push_back({ (const char *) p, bytes ? bytes : 1, g_ord++ }); }
    return p;
}
void stub_release(void * p) {
    if (p && trace_file()) {
        std::lock_guard<std::mutex> lock(g_mu);
        for (size_t i = 0; i < g_blocks.size(); ++i)
            if (g_blocks[i].base == p) { g_blocks.erase(g_blocks.begin() + i); break; }
    }
    free(p);
}
void tr(FILE * f, const void * p) {
    if (!p) { fputs(" 0", f); return; }
    for (const stub_block & b : g_blocks)
        if ((const char *) p >= b.base && (const char *) p < b.base + b.bytes) { fprintf(f, " %ld+%zu", b.ord, (size_t) ((const char *) p - b.base)); return; }
    fputs(" ?", f);
}
template <class T> std::enable_if_t<std::is_integral_v<T>> tr(FILE * f, T v) { fprintf(f, " %lld", (long long) v); }
void tr(FILE * f, float v) { fprintf(f, " %.9g", v); }
void tr(FILE * f, const qmm_tensor * t) {
    if (!t) { fputs(" [null]", f); return; }
    fprintf(f, " [t%d f%d ne", t->type, t->flags);
    for (int i = 0; i < 4; ++i) fprintf(f, " %lld", (long long) t->ne[i]);
    fputs(" nb", f);
    for (int i = 0; i < 4; ++i) fprintf(f, " %lld", (long long) t->nb[i]);
    fputs(" op", f);
    for (int i = 0; i < 16; ++i) fprintf(f, " %x", (unsigned) t->op_params[i]);
    fputs(" data", f);
    tr(f, (const void *) t->data);
    fputs("]", f);
}
void tr(FILE * f, const qmm_weight * ws, int n) {
    for (int i = 0; ws && i < n; ++i) {
        fprintf(f, " {type %d row_bytes %lld M %lld ldd %lld w", ws[i].type, (long long) ws[i].w_row_bytes, (long long) ws[i].M, (long long) ws[i].ldd);
        tr(f, ws[i].w);  fputs(" dst", f);  tr(f, (const void *) ws[i].dst);  fputs("}", f);
    }
}
void tr(FILE * f, const qmm_mv_extra * e) {
    if (!e) { fputs(" {null}", f); return; }
    fprintf(f, " {eps %.9g swiglu %d add_ld %lld sum_ld %lld norm_w", e->norm_eps, e->swiglu, (long long) e->norm_add_ld, (long long) e->norm_sum_ld);
    tr(f, (const void *) e->norm_w);  fputs(" residual", f);
    for (int i = 0; i < 4; ++i) tr(f, (const void *) e->residual[i]);
    fputs(" add", f);  tr(f, (const void *) e->norm_add);  fputs(" sum", f);  tr(f, (const void *) e->norm_sum);  fputs("}", f);
}
} // namespace
"""


def trace_stmt(name, args):
    """the statement that writes one trace line for entry point `name`; the stream is the one argument left out"""
    parts = []
    for a in args.split(","):
        a = a.strip()
        arg = re.split(r"[\s\*]+", a)[-1]
        if a == "void * stream":
            continue
        if a.startswith("const qmm_weight *"):
            parts.append(f"tr(f, {arg}, n_weights);")
        elif "*" in a and not re.match(r"const (qmm_tensor|qmm_mv_extra) \*", a):
            parts.append(f"tr(f, (const void *) {arg});")
        else:
            parts.append(f"tr(f, {arg});")
    return ('if (FILE * f = trace_file()) { std::lock_guard<std::mutex> lock(g_mu); fputs("' + name + '", f); ' + " ".join(parts) +
            ' fputc(\'\\n\', f); fflush(f); } ')


out = ["// qmm_stub.cpp — GENERATED by tests/cpp/make_qmm_stub.py from include/ggml_mi355x_{qmm,ops}.h: the C-ABI with host memory behind the",
       "// pointers and NO compute (every launch returns success, every *_supported says yes).  It exists so that the plugin's HOST logic",
       "// (csrc/ggml-mi355x.cpp: graph analysis, fusion matching, hoists, redirects, the planar-weight bookkeeping, split buffers) can run",
       "// under AddressSanitizer / UBSan in the CPU-only container (tests/test_host_sanitizers.py), where no HIP device exists.",
       "// Test infrastructure only; never linked into the product.",
       "// QMM_STUB_TRACE=<file>: every launch and every *_supported probe appends one line to <file>: its name, then its arguments.  A qmm_tensor",
       "// is written as [type flags ne nb op_params data]; a pointer as <ordinal of the qmm_malloc block that holds it>+<offset>, 0 when null, ?",
       "// when no block holds it, so the text does not depend on where malloc put things.  Unset: nothing is recorded or written.",
       '#include "ggml_mi355x_qmm.h"', '#include "ggml_mi355x_ops.h"', "#include <cstdio>", "#include <cstdlib>", "#include <cstring>", "#include <mutex>", "#include <type_traits>", "#include <vector>", "",
       TRACE_SUPPORT, 'extern "C" {', ""]
for h in ("ggml_mi355x_qmm.h", "ggml_mi355x_ops.h"):
    s = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / h).read_text(), flags=re.S)
    for m in re.finditer(r"QMM_API\s+([\w\s\*]+?)\b(qmm_\w+)\s*\(([^;]*?)\)\s*;", s, flags=re.S):
        ret, name, args = m.group(1).strip(), m.group(2), " ".join(m.group(3).split())
        body = special.get(name) or ("return 1;" if name.endswith("_supported") else "" if ret == "void" else "return nullptr;" if "*" in ret else "return 0;")
        if name not in special and (name.endswith("_supported") or "void * stream" in args):
            body = trace_stmt(name, args) + body
        out.append(f"{ret} {name}({args}) {{ {body} }}")
out += ["", '} // extern "C"', ""]
(ROOT / "tests" / "cpp" / "qmm_stub.cpp").write_text("\n".join(out))
