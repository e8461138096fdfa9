// extern "C" surface of libcunvsm_amd_testhooks.so — include/cunvsm_amd_test_hooks.h: entry points for the UNIT TESTS of single
// kernels (GEMM variants, the row sort, the gather-mean), two profiling aids (a spin kernel in front of a step, the three-launch form
// of the table passes) and the timing loops of tools/exp/. Not part of the drop-in surface and not in libcunvsm_amd.so:
// this library is loaded BEHIND the product library (RTLD_GLOBAL) and calls the product's own launchers — it carries no kernel and
// no copy of the engine, so what the hooks exercise is the code the product ships.
#include <algorithm>
#include <cstring>
#include <vector>
#include <string>

#include "c_api_internal.h"
#include "../../include/cunvsm_amd_test_hooks.h"

using cunvsm::Error;
using cunvsm::guarded_hook;
using cunvsm::guarded_on;

// kernels.h "lazy dense decay": nobody falls further behind than the factor ring is long - and the row pass and the gather do not
// clamp: a row further behind would read a stale slot of the ring
static void require_lags(const char* who, const int32_t* stamp, int64_t rows, int now) {
    for (int64_t r = 0; r < rows; ++r)
        if (stamp[r] < 0 || stamp[r] > now || now - stamp[r] > cunvsm::kLazyHistory)
            throw Error(NVSM_ERR_INVALID_ARGUMENT, std::string(who) + ": a row lags further behind than the lazy decay contract allows");
}

extern "C" {

int nvsm_debug_set_table_pass_form(int one_launch) { cunvsm::set_table_pass_one_launch(one_launch != 0); return NVSM_OK; }
int nvsm_debug_delay(nvsm_model* m, int microseconds) { NVSM_REQUIRE(m); return guarded_on(m, [&] { m->impl.debug_delay(microseconds); }); }

// nvsm_neighbors' scan through rank_scan_plain_kernel whatever the dimension (tools/bench_neighbors.py: the MFMA scan with the tail
// chunk against the plain scan on the same table, call by call). Process-wide, like the table-pass form above.
int nvsm_debug_neighbors_force_plain(int on) { cunvsm::set_nbr_scan_force_plain(on != 0); return NVSM_OK; }

// ---- debug hooks (tests only) ----
int nvsm_debug_gemm(int variant, int M, int N, int K, const float* hostA, const float* hostB, float* hostC) {
    NVSM_REQUIRE(hostA); NVSM_REQUIRE(hostB); NVSM_REQUIRE(hostC);
    return guarded_hook([&] {
        const int al = (variant >> 1) & 1, bl = variant & 1;
        const bool exact = (variant >> 30) & 1;               // bit 30: the exact-fp32 tiled kernel even where the planes kernel covers the shape
        const bool wave = (variant >> 29) & 1;                // bit 29: the projection-gradient shape on the wave-sized kernel (gemm_dtw.hip)
        const int split = (variant & 0x1fffffff) >> 2;        // variant bits: [exact << 30 | wave << 29 | split_k want << 2 | a_layout << 1 | b_layout]
        cunvsm::DevBuf<float> A, B, C, P;
        A.alloc(static_cast<size_t>(M) * K); B.alloc(static_cast<size_t>(K) * N); C.alloc(static_cast<size_t>(M) * N);
        NVSM_HIP_CHECK(hipMemcpy(A.p, hostA, A.n * sizeof(float), hipMemcpyHostToDevice));
        NVSM_HIP_CHECK(hipMemcpy(B.p, hostB, B.n * sizeof(float), hipMemcpyHostToDevice));
        const int lda = al ? M : K, ldb = bl ? K : N;
        if (split >= 1 && al == 1 && bl == 0 && wave) {
            if (!cunvsm::gemm_dtw_covers(M, N, K)) throw Error(NVSM_ERR_UNSUPPORTED, "gemm_dtw does not cover the shape");
            const int slabs = cunvsm::gemm_dtw_slabs(K, split);
            P.alloc(static_cast<size_t>(slabs) * M * N);
            if (!cunvsm::launch_gemm_dtw(A.p, B.p, slabs == 1 ? C.p : P.p, M, N, K, lda, ldb, split, nullptr)) throw Error(NVSM_ERR_UNSUPPORTED, "gemm_dtw refused a covered shape");
            if (slabs > 1) cunvsm::launch_splitk_reduce(P.p, slabs, static_cast<size_t>(M) * N, C.p, static_cast<int64_t>(M) * N, nullptr);
            NVSM_HIP_CHECK(hipDeviceSynchronize());
        } else if (split >= 1 && al == 1 && bl == 0 && !exact && cunvsm::gemm_dt_covers(M, N, K)) {
            // the projection-gradient shape: the split-bf16 split-K kernel the model uses for it (gemm_dt.hip)
            const int slabs = cunvsm::gemm_dt_slabs(K, split);
            P.alloc(static_cast<size_t>(slabs) * M * N);
            if (!cunvsm::launch_gemm_dt(A.p, B.p, P.p, M, N, K, lda, ldb, split, nullptr)) throw Error(NVSM_ERR_UNSUPPORTED, "gemm_dt refused a covered shape");
            cunvsm::launch_splitk_reduce(P.p, slabs, static_cast<size_t>(M) * N, C.p, static_cast<int64_t>(M) * N, nullptr);
            NVSM_HIP_CHECK(hipDeviceSynchronize());
        } else if (split > 1) {
            const int slabs = cunvsm::gemm_split_k_slabs(K, split);
            P.alloc(static_cast<size_t>(slabs) * M * N);
            cunvsm::launch_gemm(al, bl, A.p, B.p, P.p, M, N, K, lda, ldb, N, 1.f, nullptr, split, static_cast<size_t>(M) * N, nullptr);
            cunvsm::launch_splitk_reduce(P.p, slabs, static_cast<size_t>(M) * N, C.p, static_cast<int64_t>(M) * N, nullptr);
        } else {
            cunvsm::DevBuf<char> planes, rplanes;
            planes.alloc(cunvsm::gemm_split_planes_bytes(N, K));
            rplanes.alloc(cunvsm::gemm_rsplit_planes_bytes(N, K));
            cunvsm::GemmSplitWs sws{planes.p, planes.n, false, rplanes.p, rplanes.n, false};
            cunvsm::launch_gemm(al, bl, A.p, B.p, C.p, M, N, K, lda, ldb, N, 1.f, nullptr, 1, 0, nullptr, nullptr, nullptr, 0.f, nullptr, false,
                                nullptr, &sws);
            NVSM_HIP_CHECK(hipDeviceSynchronize());
        }
        NVSM_HIP_CHECK(hipDeviceSynchronize());
        NVSM_HIP_CHECK(hipMemcpy(hostC, C.p, C.n * sizeof(float), hipMemcpyDeviceToHost));
    });
}

// ONE named launcher of the batch-sized projection products with any of its fused epilogues (cunvsm_amd_test_hooks.h). Every
// output starts as 0xFF bytes on the device — NaN as float and as double — so that the caller sees both "refused: nothing written"
// and "launched: every element the kernel owns written"; the planes of B are cut fresh on every call.
int nvsm_debug_gemm_epilogue(const nvsm_debug_gemm_epilogue_args* a) {
    NVSM_REQUIRE(a); NVSM_REQUIRE(a->B); NVSM_REQUIRE(a->C); NVSM_REQUIRE(a->launched);
    return guarded_hook([&] {
        const int M = a->M, N = a->N, K = a->K, bl = a->b_layout;
        const bool gather = a->table != nullptr, bn = a->sums != nullptr;
        if (M <= 0 || N <= 0 || K <= 0 || (bl != 0 && bl != 1)) throw Error(NVSM_ERR_INVALID_ARGUMENT, "gemm_epilogue: bad shape");
        if (!gather && !a->A) throw Error(NVSM_ERR_INVALID_ARGUMENT, "gemm_epilogue: A is required without the gather");
        if (gather && (!a->idx || a->window < 1 || a->table_rows < 1)) throw Error(NVSM_ERR_INVALID_ARGUMENT, "gemm_epilogue: the gather needs idx, window and table_rows");
        if (bn && a->pre && (!a->mean || !a->inv_std)) throw Error(NVSM_ERR_INVALID_ARGUMENT, "gemm_epilogue: the batch-norm backward needs mean and inv_std");
        auto fill = [](void* p, size_t bytes) { if (bytes) NVSM_HIP_CHECK(hipMemset(p, 0xFF, bytes)); };
        auto up = [](void* d, const void* h, size_t bytes) { NVSM_HIP_CHECK(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice)); };
        auto down = [](void* h, const void* d, size_t bytes) { NVSM_HIP_CHECK(hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost)); };
        const size_t MK = static_cast<size_t>(M) * K, MN = static_cast<size_t>(M) * N;
        cunvsm::DevBuf<float> A, B, C, bias, rowsq, rparts, pre, mean, inv_std, dbeta, dgamma, gbias, table, wts;
        cunvsm::DevBuf<double> stats, part, part2, bsums;
        cunvsm::DevBuf<int> arrive, idx;
        cunvsm::DevBuf<int64_t> idx64;
        A.alloc(MK); B.alloc(static_cast<size_t>(K) * N); C.alloc(MN);
        if (gather) fill(A.p, MK * sizeof(float)); else up(A.p, a->A, MK * sizeof(float));
        up(B.p, a->B, B.n * sizeof(float));
        fill(C.p, MN * sizeof(float));
        if (a->bias) { bias.alloc(N); up(bias.p, a->bias, N * sizeof(float)); }
        cunvsm::GridSumWs ws{};
        if (a->colstats) {      // sized as nvsm_debug_gemm_time sizes it, the width for the split kernel's padded columns
            ws.colgroups = 8; ws.contrib_cap = M / 16 + 512; ws.width_cap = 2 * std::max((N + 31) / 32 * 32, 160);
            ws.groups_cap = ws.contrib_cap / 16 + 1; ws.fan = 16;
            part.alloc(static_cast<size_t>(ws.colgroups) * ws.contrib_cap * ws.width_cap);
            part2.alloc(static_cast<size_t>(ws.colgroups) * ws.groups_cap * ws.width_cap);
            arrive.alloc(static_cast<size_t>(ws.colgroups) * (ws.groups_cap + 1), true);
            stats.alloc(2 * static_cast<size_t>(N));
            fill(stats.p, stats.n * sizeof(double));
            ws.part = part.p; ws.part2 = part2.p; ws.arrive = arrive.p;
        }
        const int parts_cap = cunvsm::gemm_rowsq_parts(N);
        if (a->rowsq) {
            rparts.alloc(static_cast<size_t>(parts_cap) * M); rowsq.alloc(M);
            fill(rparts.p, rparts.n * sizeof(float)); fill(rowsq.p, rowsq.n * sizeof(float));
        }
        cunvsm::BnDxFused bf{};
        if (bn) {
            bsums.alloc(2 * static_cast<size_t>(K)); up(bsums.p, a->sums, bsums.n * sizeof(double));
            dbeta.alloc(K); dgamma.alloc(K); gbias.alloc(K);
            fill(dbeta.p, K * sizeof(float)); fill(dgamma.p, K * sizeof(float)); fill(gbias.p, K * sizeof(float));
            if (a->pre) {
                pre.alloc(MK); mean.alloc(K); inv_std.alloc(K);
                up(pre.p, a->pre, MK * sizeof(float)); up(mean.p, a->mean, K * sizeof(float)); up(inv_std.p, a->inv_std, K * sizeof(float));
            }
            bf = cunvsm::BnDxFused{A.p, a->pre ? pre.p : nullptr, mean.p, inv_std.p, bsums.p, dbeta.p, dgamma.p, gbias.p, a->n_global};
        }
        cunvsm::GatherFused gf{};
        if (gather) {
            const size_t nid = static_cast<size_t>(M) * a->window;
            table.alloc(static_cast<size_t>(a->table_rows) * K); up(table.p, a->table, table.n * sizeof(float));
            idx64.alloc(nid); idx.alloc(nid); up(idx64.p, a->idx, nid * sizeof(int64_t));
            if (a->wts) { wts.alloc(nid); up(wts.p, a->wts, nid * sizeof(float)); }
            cunvsm::launch_narrow_i64(idx64.p, idx.p, static_cast<int64_t>(nid), a->table_rows, nullptr, 0, nullptr);
            gf = cunvsm::GatherFused{table.p, idx.p, a->wts ? wts.p : nullptr, a->window, nullptr};
        }
        cunvsm::DevBuf<char> planes, rplanes;
        planes.alloc(cunvsm::gemm_split_planes_bytes(N, K));
        rplanes.alloc(cunvsm::gemm_rsplit_planes_bytes(N, K));
        cunvsm::GemmSplitWs sws{planes.p, planes.n, false, rplanes.p, rplanes.n, false};
        NVSM_HIP_CHECK(hipDeviceSynchronize());
        const int lda = K, ldb = bl ? K : N, ldc = N;
        const cunvsm::GridSumWs* wsp = a->colstats ? &ws : nullptr;
        const cunvsm::BnDxFused* bnp = bn ? &bf : nullptr;
        float* rq = a->rowsq ? rparts.p : nullptr;
        int nparts = a->rowsq ? 1 : 0;
        bool launched = false;
        switch (a->kernel) {
        case NVSM_DEBUG_GEMM_ROWS:
            launched = !gather && cunvsm::launch_gemm_rows(bl, A.p, B.p, C.p, M, N, K, lda, ldb, ldc, a->alpha, bias.p, nullptr, stats.p, wsp, rq, a->rowsq_scale, bnp);
            break;
        case NVSM_DEBUG_GEMM_RSPLIT:
            launched = cunvsm::launch_gemm_rsplit(bl, A.p, B.p, C.p, M, N, K, lda, ldb, ldc, a->alpha, bias.p, nullptr, stats.p, wsp, rq, a->rowsq_scale, &sws, bnp,
                                                  gather ? &gf : nullptr);
            break;
        case NVSM_DEBUG_GEMM_SPLIT:
            launched = !gather && cunvsm::launch_gemm_split(bl, A.p, B.p, C.p, M, N, K, lda, ldb, ldc, a->alpha, bias.p, nullptr, stats.p, wsp, rq, a->rowsq_scale, &sws, bnp);
            break;
        case NVSM_DEBUG_GEMM_TSTAT:
            launched = !gather && !bn && cunvsm::launch_gemm_tstat(0, bl, A.p, B.p, C.p, M, N, K, lda, ldb, ldc, a->alpha, bias.p, nullptr, stats.p, rq, a->rowsq_scale,
                                                                   &nparts, false, wsp);
            break;
        case NVSM_DEBUG_GEMM_TILED:
            if (!gather && !bn) {      // launch_gemm with every other kernel switched off: no row-panel batch size, no planes, no LDS-stationary / panel kernel
                cunvsm::Tuning t = cunvsm::tuning();
                t.gemm_rows_max = 0;
                cunvsm::TuningScope scope(&t);
                struct Off { Off() { cunvsm::gemm_set_tstat_enabled(false); cunvsm::gemm_set_panel_enabled(false); }
                             ~Off() { cunvsm::gemm_set_tstat_enabled(true); cunvsm::gemm_set_panel_enabled(true); } } off;
                cunvsm::launch_gemm(0, bl, A.p, B.p, C.p, M, N, K, lda, ldb, ldc, a->alpha, bias.p, 1, 0, nullptr, stats.p, rq, a->rowsq_scale, &nparts, false, wsp, nullptr);
                launched = true;
            }
            break;
        default: throw Error(NVSM_ERR_INVALID_ARGUMENT, "gemm_epilogue: kernel 0 = rows, 1 = rsplit, 2 = split, 3 = tstat, 4 = tiled");
        }
        NVSM_HIP_CHECK(hipGetLastError());
        if (launched && a->rowsq && nparts > 1) cunvsm::launch_sum_parts(rparts.p, nparts, M, rowsq.p, M, nullptr);
        NVSM_HIP_CHECK(hipDeviceSynchronize());
        *a->launched = launched ? 1 : 0;
        down(a->C, C.p, MN * sizeof(float));
        if (a->A_out) down(a->A_out, A.p, MK * sizeof(float));
        if (a->colstats) down(a->colstats, stats.p, stats.n * sizeof(double));
        if (a->rowsq) down(a->rowsq, (launched && nparts > 1) ? rowsq.p : rparts.p, M * sizeof(float));
        if (bn) {
            if (a->dbeta) down(a->dbeta, dbeta.p, K * sizeof(float));
            if (a->dgamma) down(a->dgamma, dgamma.p, K * sizeof(float));
            if (a->grad_bias) down(a->grad_bias, gbias.p, K * sizeof(float));
        }
    });
}

// What a launcher of nvsm_debug_gemm_epilogue would do with (shape, epilogue) — host arithmetic only, no HIP call: *covers and the
// plan word of cunvsm_amd_test_hooks.h. The answers come from the functions the launchers themselves decide by (kernels.h).
int nvsm_debug_gemm_plan(int kernel, int b_layout, int M, int N, int K, int flags, int window, int* covers, unsigned* plan) {
    NVSM_REQUIRE(covers); NVSM_REQUIRE(plan);
    return guarded_hook([&] {
        const bool colstats = flags & NVSM_DEBUG_EPI_COLSTATS, rowsq = flags & NVSM_DEBUG_EPI_ROWSQ, bn = flags & NVSM_DEBUG_EPI_BN;
        const bool bias = flags & NVSM_DEBUG_EPI_BIAS, gather = flags & NVSM_DEBUG_EPI_GATHER, gb = flags & NVSM_DEBUG_EPI_BIAS_GRAD;
        *covers = 0; *plan = 0;
        if (M <= 0 || N <= 0 || K <= 0 || (b_layout != 0 && b_layout != 1) || (bn && gb)) return;
        if (gather && kernel != NVSM_DEBUG_GEMM_RSPLIT) return;
        switch (kernel) {
        case NVSM_DEBUG_GEMM_ROWS: {
            int tpw = 0, waves = 0;
            if (!cunvsm::gemm_rows_plan(b_layout, M, N, K, colstats, rowsq, bn, &tpw, &waves)) return;
            *plan = static_cast<unsigned>(waves | (tpw << 8));
            break;
        }
        case NVSM_DEBUG_GEMM_RSPLIT: {
            cunvsm::RsplitPlan p;
            if (gather && window < 1) return;
            if (!cunvsm::gemm_rsplit_plan(b_layout, M, N, K, colstats, rowsq, bn, gather ? window : 0, &p)) return;
            *plan = static_cast<unsigned>(p.waves | (p.rch << 8) | ((p.ksp != p.ks ? 1 : 0) << 16) | ((N - 32 * (p.nt - 1)) << 24));
            break;
        }
        case NVSM_DEBUG_GEMM_SPLIT: {
            cunvsm::SplitPlan p;
            if (!cunvsm::gemm_split_plan(b_layout, M, N, K, colstats, rowsq, bias, bn || gb, &p)) return;
            *plan = static_cast<unsigned>(p.cbs | (p.ncb_min << 8) | (p.ncb_max << 16));
            break;
        }
        case NVSM_DEBUG_GEMM_TSTAT: {
            cunvsm::TstatPlan p;
            if (bn || gb) return;          // (launch_gemm_tstat has no argument for either: nvsm_debug_gemm_epilogue does not call it then)
            if (!cunvsm::gemm_tstat_plan(b_layout, M, N, K, colstats, rowsq, bias, &p)) return;
            *plan = static_cast<unsigned>(p.parts | (p.NT << 8) | ((p.mixed ? 1 : 0) << 16) | (p.KG << 24));
            break;
        }
        case NVSM_DEBUG_GEMM_TILED:
            if (bn || gb) return;
            break;
        default: throw Error(NVSM_ERR_INVALID_ARGUMENT, "gemm_plan: kernel 0 = rows, 1 = rsplit, 2 = split, 3 = tstat, 4 = tiled");
        }
        *covers = 1;
    });
}

// The round layout of the retrieval calls (cunvsm_amd_test_hooks.h) — host arithmetic only, no HIP call: the answer of the function
// the rounds of ranking.cpp themselves call.
int nvsm_debug_rank_layout(int64_t rows, int64_t k, int64_t queries, int64_t slab_mb, int64_t slab_cap, const int64_t* lengths, int64_t* out) {
    NVSM_REQUIRE(out);
    return guarded_hook([&] {
        if (queries < 1 || (!lengths && (rows < 1 || k < 1 || k > rows || slab_mb < 1 || slab_cap < 0))) throw Error(NVSM_ERR_INVALID_ARGUMENT, "rank_layout: bad sizes");
        std::vector<int64_t> off(lengths ? static_cast<size_t>(queries) + 1 : 0, 0);
        for (size_t i = 1; i < off.size(); ++i) off[i] = off[i - 1] + lengths[i - 1];
        const cunvsm::RankLayout l = lengths ? cunvsm::rank_layout_candidates(off.data(), queries) : cunvsm::rank_layout(rows, k, queries, slab_mb << 18, slab_cap);
        out[0] = l.qn; out[1] = l.S; out[2] = l.ld; out[3] = l.n_keys; out[4] = l.npad;
    });
}

// average milliseconds of one launch_gemm of the batch-sized products on device-resident operands (A [M][K], B per b_layout):
// extras bit 0 = ordered column statistics (the forward product), bit 1 = row sums of squares (the backward one)
int nvsm_debug_gemm_time(int b_layout, int M, int N, int K, int extras, int repeats, float* avg_ms) {
    NVSM_REQUIRE(avg_ms);
    return guarded_hook([&] {
        cunvsm::DevBuf<float> A, B, C, rowsq;
        cunvsm::DevBuf<double> stats, part, part2;
        cunvsm::DevBuf<int> arrive;
        A.alloc(static_cast<size_t>(M) * K); B.alloc(static_cast<size_t>(K) * N); C.alloc(static_cast<size_t>(M) * N);
        {   // operands with all 24 significant bits in use (zeros would flatter a kernel: less switching, higher clocks)
            std::vector<float> h(std::max(A.n, B.n));
            uint32_t x = 12345u;
            auto fill = [&](cunvsm::DevBuf<float>& d, float scale) {
                for (size_t i = 0; i < d.n; ++i) { x = x * 1664525u + 1013904223u; h[i] = (static_cast<float>(x >> 8) * (1.f / 8388608.f) - 1.f) * scale; }
                NVSM_HIP_CHECK(hipMemcpy(d.p, h.data(), d.n * sizeof(float), hipMemcpyHostToDevice));
            };
            fill(A, 0.5f); fill(B, 0.1f);
        }
        cunvsm::GridSumWs ws{};
        if (extras & 1) {
            ws.colgroups = 8; ws.contrib_cap = M / 32 + 512; ws.width_cap = 2 * (N > 160 ? N : 160); ws.groups_cap = ws.contrib_cap / 16 + 1; ws.fan = 16;
            part.alloc(static_cast<size_t>(ws.colgroups) * ws.contrib_cap * ws.width_cap);
            part2.alloc(static_cast<size_t>(ws.colgroups) * ws.groups_cap * ws.width_cap);
            arrive.alloc(static_cast<size_t>(ws.colgroups) * (ws.groups_cap + 1), true);
            stats.alloc(2 * static_cast<size_t>(N), true);
            ws.part = part.p; ws.part2 = part2.p; ws.arrive = arrive.p;
        }
        if (extras & 2) rowsq.alloc(static_cast<size_t>(M) * cunvsm::gemm_rowsq_parts(N));
        hipStream_t s;
        NVSM_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        hipEvent_t e0, e1;
        NVSM_HIP_CHECK(hipEventCreate(&e0)); NVSM_HIP_CHECK(hipEventCreate(&e1));
        const int ldb = b_layout ? K : N;
        int parts = 0;
        cunvsm::DevBuf<char> planes, rplanes;
        planes.alloc(cunvsm::gemm_split_planes_bytes(N, K));
        rplanes.alloc(cunvsm::gemm_rsplit_planes_bytes(N, K));
        cunvsm::GemmSplitWs sws{planes.p, planes.n, false, rplanes.p, rplanes.n, false};
        auto go = [&] {
            sws.ready = (extras & 4) != 0 && sws.ready;          // extras bit 2: the planes of B stay valid between launches
            sws.rready = (extras & 4) != 0 && sws.rready;
            cunvsm::launch_gemm(0, b_layout, A.p, B.p, C.p, M, N, K, K, ldb, N, 1.f, nullptr, 1, 0, s, (extras & 1) ? stats.p : nullptr,
                                (extras & 2) ? rowsq.p : nullptr, 1.f, &parts, false, (extras & 1) ? &ws : nullptr, &sws);
        };
        for (int i = 0; i < 3; ++i) go();
        NVSM_HIP_CHECK(hipEventRecord(e0, s));
        for (int i = 0; i < repeats; ++i) go();
        NVSM_HIP_CHECK(hipEventRecord(e1, s));
        NVSM_HIP_CHECK(hipEventSynchronize(e1));
        float ms = 0.f;
        NVSM_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        *avg_ms = ms / static_cast<float>(repeats > 0 ? repeats : 1);
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipStreamDestroy(s);
    });
}

// the dT product alone on device-resident operands (phrase [rows][M], dx [rows][N]): average ms of the split-K kernel and of
// the reduce behind it. which 0 = gemm_dt (split-bf16), 2 = the tiled exact-fp32 kernel
int nvsm_debug_dt_time(int M, int N, int rows, int slabs, int repeats, int which, float* kernel_ms, float* reduce_ms) {
    NVSM_REQUIRE(kernel_ms); NVSM_REQUIRE(reduce_ms);
    return guarded_hook([&] {
        cunvsm::DevBuf<float> A, B, C, P;
        A.alloc(static_cast<size_t>(rows) * M); B.alloc(static_cast<size_t>(rows) * N); C.alloc(static_cast<size_t>(M) * N);
        {
            std::vector<float> h(std::max(A.n, B.n));
            uint32_t x = 4242u;
            auto fill = [&](cunvsm::DevBuf<float>& d, float scale) {
                for (size_t i = 0; i < d.n; ++i) { x = x * 1664525u + 1013904223u; h[i] = (static_cast<float>(x >> 8) * (1.f / 8388608.f) - 1.f) * scale; }
                NVSM_HIP_CHECK(hipMemcpy(d.p, h.data(), d.n * sizeof(float), hipMemcpyHostToDevice));
            };
            fill(A, 0.5f); fill(B, 0.1f);
        }
        hipStream_t s;
        NVSM_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        if (which != 0 && which != 1 && which != 2) throw Error(NVSM_ERR_INVALID_ARGUMENT, "which: 0 = split-bf16 kernel, 1 = its wave-sized form, 2 = tiled fp32 kernel");
        const int ns = which == 0 ? cunvsm::gemm_dt_slabs(rows, slabs) : (which == 1 ? cunvsm::gemm_dtw_slabs(rows, slabs) : cunvsm::gemm_split_k_slabs(rows, slabs));
        const size_t stride = static_cast<size_t>(M) * N;
        P.alloc(static_cast<size_t>(std::max(ns, 1)) * stride);
        auto product = [&] {
            bool ok = true;
            if (which == 0) ok = cunvsm::launch_gemm_dt(A.p, B.p, P.p, M, N, rows, M, N, slabs, s);
            else if (which == 1) ok = cunvsm::launch_gemm_dtw(A.p, B.p, P.p, M, N, rows, M, N, slabs, s);
            else cunvsm::launch_gemm(1, 0, A.p, B.p, P.p, M, N, rows, M, N, N, 1.f, nullptr, slabs, stride, s);
            if (!ok) throw Error(NVSM_ERR_UNSUPPORTED, "the dT kernel refused the shape");
        };
        auto reduce = [&] { cunvsm::launch_splitk_reduce(P.p, ns, stride, C.p, static_cast<int64_t>(stride), s); };
        hipEvent_t e0, e1, e2;
        NVSM_HIP_CHECK(hipEventCreate(&e0)); NVSM_HIP_CHECK(hipEventCreate(&e1)); NVSM_HIP_CHECK(hipEventCreate(&e2));
        for (int i = 0; i < 3; ++i) { product(); reduce(); }
        const int reps = repeats > 0 ? repeats : 1;
        NVSM_HIP_CHECK(hipEventRecord(e0, s));
        for (int i = 0; i < reps; ++i) product();
        NVSM_HIP_CHECK(hipEventRecord(e1, s));
        for (int i = 0; i < reps; ++i) reduce();
        NVSM_HIP_CHECK(hipEventRecord(e2, s));
        NVSM_HIP_CHECK(hipEventSynchronize(e2));
        float a = 0.f, b = 0.f;
        NVSM_HIP_CHECK(hipEventElapsedTime(&a, e0, e1)); NVSM_HIP_CHECK(hipEventElapsedTime(&b, e1, e2));
        *kernel_ms = a / reps; *reduce_ms = b / reps;
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipEventDestroy(e2); (void)hipStreamDestroy(s);
    });
}

int nvsm_debug_sort(int64_t n, int bits, const int32_t* keys, int32_t* keys_out, int32_t* vals_out, int repeats, float* avg_ms) {
    NVSM_REQUIRE(keys); NVSM_REQUIRE(keys_out); NVSM_REQUIRE(vals_out);
    return guarded_hook([&] {
        if (n <= 0) return;
        cunvsm::DevBuf<int> K, KO, VO;
        cunvsm::DevBuf<char> tmp;
        K.alloc(n); KO.alloc(n); VO.alloc(n);
        const size_t tb = cunvsm::sort_pairs_temp_bytes(n, bits);
        tmp.alloc(tb, true);
        int* err = nullptr;
        NVSM_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&err), sizeof(int), hipHostMallocDefault));
        *err = 0;
        uint64_t epoch = 0;
        NVSM_HIP_CHECK(hipMemcpy(K.p, keys, n * sizeof(int), hipMemcpyHostToDevice));
        hipEvent_t e0, e1;
        NVSM_HIP_CHECK(hipEventCreate(&e0)); NVSM_HIP_CHECK(hipEventCreate(&e1));
        cunvsm::sort_pairs(tmp.p, tb, &epoch, K.p, KO.p, nullptr, VO.p, n, bits, err, nullptr);      // warm-up
        NVSM_HIP_CHECK(hipEventRecord(e0, nullptr));
        const int reps = repeats > 0 ? repeats : 1;
        for (int r = 0; r < reps; ++r)      // repeats: the arrival counter keeps growing across calls
            cunvsm::sort_pairs(tmp.p, tb, &epoch, K.p, KO.p, nullptr, VO.p, n, bits, err, nullptr);
        NVSM_HIP_CHECK(hipEventRecord(e1, nullptr));
        NVSM_HIP_CHECK(hipDeviceSynchronize());
        float ms = 0.f;
        NVSM_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (avg_ms) *avg_ms = ms / reps;
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        const int code = *err;
        (void)hipHostFree(err);
        if (code) throw Error(NVSM_ERR_DEVICE, "sort reported an error");
        NVSM_HIP_CHECK(hipMemcpy(keys_out, KO.p, n * sizeof(int), hipMemcpyDeviceToHost));
        NVSM_HIP_CHECK(hipMemcpy(vals_out, VO.p, n * sizeof(int), hipMemcpyDeviceToHost));
    });
}

// One table pass on caller-supplied inputs (cunvsm_amd_test_hooks.h): the workspace of Model::alloc_table_csr / alloc_table with one
// index set, the launch sequence of Model::build_csr, the arguments of Model::update_words / update_entities.
int nvsm_debug_table_pass(const nvsm_debug_table_pass_args* a) {
    NVSM_REQUIRE(a); NVSM_REQUIRE(a->X);
    return cunvsm::guarded([&] {
        using namespace cunvsm;
        const int64_t rows = a->rows, n = a->n, prev_n = a->prev_keys ? a->prev_n : 0, cap = a->max_entries;
        const int dim = a->dim, kind = a->kind;
        const bool adam = a->adam != 0, order = a->chunk_order != 0, lazy = a->stamp != nullptr;
        const bool uses_m = kind == ROW_ADAM_MV || kind == ROW_ADAM_SPARSE_ENT || kind == ROW_ADAM_DENSE || kind == ROW_ADAM_FULL;
        const bool uses_p = kind == ROW_SGD || kind == ROW_ADAGRAD_ENT || kind == ROW_ADAM_SPARSE_ENT || kind == ROW_ADAM_DENSE || kind == ROW_ADAM_FULL;
        const bool uses_sc = kind == ROW_ADAGRAD_ENT || kind == ROW_SCALAR_ACC || kind == ROW_ADAM_MV || kind == ROW_ADAM_SPARSE_ENT || kind == ROW_ADAM_DENSE;
        auto bad = [](const char* what) { throw Error(NVSM_ERR_INVALID_ARGUMENT, std::string("table_pass: ") + what); };
        if ((a->table != 0 && a->table != 1) || kind < ROW_SGD || kind > ROW_SCALAR_ACC) bad("table 0 / 1, kind 0 .. 6");
        if (rows < 1 || rows >= (int64_t(1) << 30) || dim < 1 || n < 0 || prev_n < 0 || cap < 1 || n > cap || prev_n > cap) bad("bad sizes");
        if (cap >= (int64_t(1) << 26) || a->div < 1 || a->div > 2048 || a->num_src < 1 || std::max(n, prev_n) > a->num_src * a->div) bad("entries must map to source rows: e / div < num_src, e < 2^26");
        if ((n > 0 && !a->keys) || (uses_p && !a->P) || (uses_m && !a->m) || (kind == ROW_ADAM_FULL && !a->v) || (uses_sc && (!a->sc_in || !a->sc_out))) bad("a state array the kind needs is null");
        if (a->table == 1 && a->src_scale) bad("src_scale belongs to the words table");
        for (int64_t i = 0; i < n; ++i) if (a->keys[i] < 0 || a->keys[i] >= rows) bad("key out of range");
        for (int64_t i = 0; i < prev_n; ++i) if (a->prev_keys[i] < 0 || a->prev_keys[i] >= rows) bad("previous key out of range");
        if (lazy) {
            if (kind == ROW_ADAM_DENSE || kind == ROW_ADAM_FULL || kind == ROW_SCALAR_ACC) throw Error(NVSM_ERR_UNSUPPORTED, "table_pass: the model never runs this kind with pending decay");
            if (!a->lazy_decay || !a->stamp_out) bad("pending decay needs the factor ring and stamp_out");
            if (prev_n > 0) bad("pending decay and a previous batch do not go together");
            require_lags("table_pass", a->stamp, rows, a->now);
        }

        // the form of the pass: these fields and the defaults, whatever the environment says
        Tuning t;
        t.csr_fill_in_bounds = a->fill_in_bounds != 0;
        t.entry_walk_min = a->entry_walk_min;
        TuningScope scope(&t);
        struct Form { bool was; explicit Form(bool on) : was(table_pass_one_launch()) { set_table_pass_one_launch(on); }
                      ~Form() { set_table_pass_one_launch(was); } } form(a->one_launch != 0);

        auto up = [](void* d, const void* h, size_t bytes) { if (bytes) NVSM_HIP_CHECK(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice)); };
        auto down = [](void* h, const void* d, size_t bytes) { if (bytes) NVSM_HIP_CHECK(hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost)); };
        auto copy = [](void* d, const void* s, size_t bytes) { if (bytes) NVSM_HIP_CHECK(hipMemcpy(d, s, bytes, hipMemcpyDeviceToDevice)); };
        const size_t RD = static_cast<size_t>(rows) * dim, nent = static_cast<size_t>(std::max(n, prev_n));

        // ---- the workspace, as Model::alloc_table_csr / alloc_table size it ----
        int max_chunks = 0, max_chunks2 = 0;
        csr_chunk_caps(adam, dim, cap, &max_chunks, &max_chunks2);
        DevBuf<int> sorted_key, sorted_entry, csr_zeroed, chunk_base, touched, chunk_desc, chunk2_base, chunk2_desc, chunk_order, chunk_key,
            chunk_key_sorted, arrive_row, arrive2, keys, prev_keys;
        DevBuf<float> partial, partial_q, partial2, partial2_q;
        DevBuf<char> sort_temp;
        sorted_key.alloc(cap); sorted_entry.alloc(cap);
        csr_zeroed.alloc(csr_counter_ints(rows), true); chunk_base.alloc(rows, true);
        touched.alloc(std::min<int64_t>(rows, cap));
        chunk_desc.alloc(static_cast<size_t>(max_chunks) * 3, true);
        chunk2_base.alloc(rows, true);
        chunk2_desc.alloc(static_cast<size_t>(max_chunks2) * 2, true);
        if (order) { chunk_order.alloc(max_chunks, true); chunk_key.alloc(max_chunks, true); chunk_key_sorted.alloc(max_chunks, true); }
        partial.alloc(static_cast<size_t>(max_chunks) * dim); partial_q.alloc(max_chunks);
        partial2.alloc(static_cast<size_t>(max_chunks2) * dim); partial2_q.alloc(max_chunks2);
        NVSM_HIP_CHECK(hipMemset(partial.p, 0xFF, partial.n * sizeof(float))); NVSM_HIP_CHECK(hipMemset(partial_q.p, 0xFF, partial_q.n * sizeof(float)));
        NVSM_HIP_CHECK(hipMemset(partial2.p, 0xFF, partial2.n * sizeof(float))); NVSM_HIP_CHECK(hipMemset(partial2_q.p, 0xFF, partial2_q.n * sizeof(float)));
        arrive2.alloc(max_chunks2, true); arrive_row.alloc(rows, true);
        int sort_bits = 1;
        while ((int64_t(1) << sort_bits) < rows) ++sort_bits;
        const size_t sort_temp_bytes = sort_pairs_temp_bytes(cap, sort_bits);
        sort_temp.alloc(sort_temp_bytes, true);

        // ---- inputs and state ----
        DevBuf<float> X, coef, sq_src, src_scale, P, m, v, sc_in, sc_out, P2, m2, v2, sc2_in, sc2_out;
        X.alloc(static_cast<size_t>(a->num_src) * dim); up(X.p, a->X, X.n * sizeof(float));
        if (a->coef) { coef.alloc(nent); up(coef.p, a->coef, nent * sizeof(float)); }
        if (a->sq_src) { sq_src.alloc(a->num_src); up(sq_src.p, a->sq_src, sq_src.n * sizeof(float)); }
        if (a->src_scale) { src_scale.alloc(a->num_src); up(src_scale.p, a->src_scale, src_scale.n * sizeof(float)); }
        const bool in_place = uses_sc && (lazy || a->sc_out == a->sc_in);      // (lazy: sc_in uploads the stored scalar, written in place)
        DevBuf<int> stamp;
        DevBuf<float> snapshot;
        if (lazy) {
            stamp.alloc(rows); up(stamp.p, a->stamp, rows * sizeof(int));
            if (uses_sc) { snapshot.alloc(rows); NVSM_HIP_CHECK(hipMemset(snapshot.p, 0xFF, rows * sizeof(float))); }
        }
        if (a->P) { P.alloc(RD); up(P.p, a->P, RD * sizeof(float)); }
        if (a->m) { m.alloc(RD); up(m.p, a->m, RD * sizeof(float)); }
        if (a->v) { v.alloc(RD); up(v.p, a->v, RD * sizeof(float)); }
        if (a->sc_in) { sc_in.alloc(rows); up(sc_in.p, a->sc_in, rows * sizeof(float)); }
        if (a->sc_out && !in_place) { sc_out.alloc(rows); up(sc_out.p, a->sc_out, rows * sizeof(float)); }
        if (n > 0) { keys.alloc(n); up(keys.p, a->keys, n * sizeof(int)); }
        if (prev_n > 0) {
            prev_keys.alloc(prev_n); up(prev_keys.p, a->prev_keys, prev_n * sizeof(int));
            if (P.p) { P2.alloc(RD); copy(P2.p, P.p, RD * sizeof(float)); }
            if (m.p) { m2.alloc(RD); copy(m2.p, m.p, RD * sizeof(float)); }
            if (v.p) { v2.alloc(RD); copy(v2.p, v.p, RD * sizeof(float)); }
            if (sc_in.p) { sc2_in.alloc(rows); copy(sc2_in.p, sc_in.p, rows * sizeof(float)); }
            if (sc_out.p) { sc2_out.alloc(rows); copy(sc2_out.p, sc_out.p, rows * sizeof(float)); }
        }

        hipStream_t s;
        NVSM_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        int* err = nullptr;
        NVSM_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&err), sizeof(int), hipHostMallocDefault));
        *err = 0;
        uint64_t epoch = 0;
        NVSM_HIP_CHECK(hipDeviceSynchronize());

        auto run = [&](const int* k, int64_t cnt, float* tp, float* tm, float* tv, const float* si, float* so) {
            Csr c{};
            c.sorted_key = sorted_key.p; c.sorted_entry = sorted_entry.p;
            c.row_begin = csr_zeroed.p; c.row_end = csr_zeroed.p + rows; c.chunk_base = chunk_base.p;
            c.chunk_desc = chunk_desc.p; c.num_chunks = csr_zeroed.p + 2 * rows;
            c.num_touched = c.num_chunks + 2; c.touched = touched.p;
            c.partial = partial.p; c.partial_q = partial_q.p;
            c.chunk2_base = chunk2_base.p; c.chunk2_desc = chunk2_desc.p; c.chunk_order = chunk_order.p;
            c.partial2 = partial2.p; c.partial2_q = partial2_q.p;
            c.arrive_row = arrive_row.p; c.arrive2 = arrive2.p;
            c.n = cnt; c.rows = rows; c.max_chunks = max_chunks; c.max_chunks2 = max_chunks2;
            c.chunk = csr_chunk_entries(adam, dim, cnt);
            // Model::build_csr
            sort_pairs(sort_temp.p, sort_temp_bytes, &epoch, k, sorted_key.p, nullptr, sorted_entry.p, cnt, sort_bits, err, s,
                       csr_zeroed.p, csr_counter_ints(rows));
            launch_csr_build(c, s, cnt > 0, chunk_order.p ? chunk_key.p : nullptr);
            if (chunk_order.p) launch_chunk_order(c, chunk_key.p, chunk_key_sorted.p, sort_temp.p, sort_temp_bytes, s, /*keys_written=*/cnt > 0);
            // Model::update_words / update_entities
            RowPassArgs r{};
            r.table = a->table; r.kind = kind; r.X = X.p;
            if (a->table == 0) r.wts = coef.p; else r.coefs = coef.p;
            r.sq_src = sq_src.p; r.src_scale = src_scale.p;
            r.div = static_cast<uint32_t>(a->div);
            r.div_magic = (uint64_t(1) << 37) / r.div + 1;
            r.P = tp; r.m = tm; r.v = tv; r.sc_in = si; r.sc_out = so; r.dim = dim;
            if (uses_m || (kind == ROW_SGD && a->wide)) fill_adam_consts(r, a->bc, a->lambda);      // (the wide SGD pass is a copy of the moments pass's arguments)
            r.lr = a->lr; r.lambda = a->lambda; r.decay = a->decay; r.eps = 1e-6f;
            r.dense = a->dense != 0; r.wide = a->wide != 0;
            r.nt_m = a->nt & 1; r.nt_p = (a->nt >> 1) & 1;
            if (lazy) {
                // Model::lazy_begin_update, Model::lazy_scalar_snapshot
                r.lazy = 1;
                r.pending.stamp = stamp.p; r.pending.now = a->now; std::memcpy(r.pending.decay, a->lazy_decay, sizeof(r.pending.decay));
                if (uses_sc) {
                    LazyRefreshArgs f{};
                    f.scalars_only = 1;
                    f.sc = so; f.sc_snapshot = snapshot.p;
                    f.stamp = stamp.p; f.rows = rows; f.dim = dim; f.now = a->now;
                    f.s_m = 1.f; f.s_v = uses_m ? r.s_v : 1.f;
                    f.list = c.touched; f.list_count = c.num_touched;
                    launch_lazy_refresh(f, std::min<int64_t>(cnt, rows), s);
                    r.sc_in = snapshot.p;
                }
            }
            const int path = launch_table_pass(c, r, s);
            if (lazy) launch_stamp_rows(c, stamp.p, a->now + 1, std::min<int64_t>(cnt, rows), s);      // Model::lazy_end_update
            NVSM_HIP_CHECK(hipGetLastError());
            NVSM_HIP_CHECK(hipStreamSynchronize(s));
            return std::make_pair(path, c.chunk);
        };
        std::pair<int, int> res{0, 0};
        try {
            if (prev_n > 0) run(prev_keys.p, prev_n, P2.p, m2.p, v2.p, sc2_in.p, in_place ? sc2_in.p : sc2_out.p);
            res = run(keys.p, n, P.p, m.p, v.p, sc_in.p, in_place ? sc_in.p : sc_out.p);
        } catch (...) {
            (void)hipStreamDestroy(s); (void)hipHostFree(err);
            throw;
        }
        const int code = *err;
        (void)hipStreamDestroy(s); (void)hipHostFree(err);
        if (code) throw Error(NVSM_ERR_DEVICE, "sort reported an error");

        if (a->path) *a->path = res.first;
        if (a->chunk) *a->chunk = res.second;
        if (a->num_chunks) down(a->num_chunks, csr_zeroed.p + 2 * rows, 2 * sizeof(int));
        if (a->max_chunks) *a->max_chunks = max_chunks;
        if (a->max_chunks2) *a->max_chunks2 = max_chunks2;
        if (a->arrive_left) {      // the arrival counters of the one-launch pass are back at zero
            std::vector<int> h(std::max<size_t>(rows, max_chunks2));
            int left = 0;
            down(h.data(), arrive_row.p, rows * sizeof(int));
            for (int64_t i = 0; i < rows; ++i) left += h[i] != 0;
            down(h.data(), arrive2.p, max_chunks2 * sizeof(int));
            for (int i = 0; i < max_chunks2; ++i) left += h[i] != 0;
            *a->arrive_left = left;
        }
        if (a->P) down(a->P, P.p, RD * sizeof(float));
        if (a->m) down(a->m, m.p, RD * sizeof(float));
        if (a->v) down(a->v, v.p, RD * sizeof(float));
        if (uses_sc) down(a->sc_out, in_place ? sc_in.p : sc_out.p, rows * sizeof(float));
        if (lazy) down(a->stamp_out, stamp.p, rows * sizeof(int));
    });
}

// One launch_loss on caller-supplied inputs (cunvsm_amd_test_hooks.h): the arguments of Model::forward's loss block — the constants
// by the same fill_loss_consts —, the grid-sum workspace as Model::alloc_sums sizes it for a batch of B, every output behind a guard.
int nvsm_debug_loss(const nvsm_debug_loss_args* a) {
    NVSM_REQUIRE(a); NVSM_REQUIRE(a->pre); NVSM_REQUIRE(a->E); NVSM_REQUIRE(a->ids);
    return cunvsm::guarded([&] {
        using namespace cunvsm;
        const int64_t B = a->B, rows = a->rows;
        const int de = a->de, R = a->R, k = a->k;
        const bool bn = a->bn != 0, lazy = a->stamp != nullptr;
        auto bad = [](const char* what) { throw Error(NVSM_ERR_INVALID_ARGUMENT, std::string("loss: ") + what); };
        if (B < 1 || B >= (int64_t(1) << 24) || R < 1 || R > 4096 || k < 0 || rows < 1 || rows >= (int64_t(1) << 31)) bad("bad sizes");
        if (de < 1 || de > 1024 || (de % 4 != 0 && de > 256)) bad("entity_dim is at most 1024, and at most 256 where it is no multiple of 4");      // (Model's own limits)
        if (bn && (!a->bn_sums || !a->bias || !(a->bn_n > 0))) bad("batch-norm needs bn_sums, bn_n and bias");
        if (!(a->b_global > 0) || a->repeats < 1 || a->rows_for_dispatch < 0) bad("b_global > 0, repeats >= 1, rows_for_dispatch >= 0");
        if (a->nonlinearity != 0 && a->nonlinearity != 1) bad("nonlinearity 0 tanh / 1 hard_tanh");
        for (int64_t i = 0; i < B * R; ++i) if (a->ids[i] < 0 || a->ids[i] >= rows) bad("id out of range");
        if (lazy) {
            if (!a->decay) bad("a lazy view needs the factor ring");
            if (!loss_reads_lazily(de, R, a->l2_entity != 0)) throw Error(NVSM_ERR_UNSUPPORTED, "loss: the kernel for this shape reads the rows as they are (the model refreshes them first)");
            for (int64_t r = 0; r < rows; ++r)      // kernels.h "lazy dense decay": nobody falls further behind than the factor ring is long
                if (a->stamp[r] < 0 || a->stamp[r] > a->now || a->now - a->stamp[r] > kLazyHistory) bad("a row lags further behind than the lazy decay contract allows");
        }

        // the dispatch by its rules, whatever the environment says
        Tuning t;
        TuningScope scope(&t);

        auto fill = [](void* p, size_t bytes) { if (bytes) NVSM_HIP_CHECK(hipMemset(p, 0xFF, bytes)); };
        auto up = [](void* d, const void* h, size_t bytes) { if (bytes) NVSM_HIP_CHECK(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice)); };
        auto down = [](void* h, const void* d, size_t bytes) { if (h && bytes) NVSM_HIP_CHECK(hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost)); };
        const size_t Bde = static_cast<size_t>(B) * de, BR = static_cast<size_t>(B) * R, sde = static_cast<size_t>(de);

        DevBuf<float> pre, bias, E, inst_w, proj, dy, coef, probs, pp, bn_mean, bn_inv_std;
        DevBuf<double> bn_sums, acc, part, part2;
        DevBuf<int> ids, stamp, arrive;
        pre.alloc(Bde); up(pre.p, a->pre, Bde * sizeof(float));
        E.alloc(static_cast<size_t>(rows) * de); up(E.p, a->E, E.n * sizeof(float));
        ids.alloc(BR); up(ids.p, a->ids, BR * sizeof(int));
        if (bn) { bn_sums.alloc(2 * sde); up(bn_sums.p, a->bn_sums, 2 * sde * sizeof(double)); }
        if (a->bias) { bias.alloc(sde); up(bias.p, a->bias, sde * sizeof(float)); }
        if (a->inst_w) { inst_w.alloc(B); up(inst_w.p, a->inst_w, B * sizeof(float)); }
        if (lazy) { stamp.alloc(rows); up(stamp.p, a->stamp, rows * sizeof(int)); }
        // outputs: one more row (R more elements) than the kernel owns, everything 0xFF
        proj.alloc(Bde + sde); dy.alloc(Bde + sde); coef.alloc(BR + R); probs.alloc(BR + R); pp.alloc(B + 1);
        bn_mean.alloc(2 * sde); bn_inv_std.alloc(2 * sde); acc.alloc(1 + 3 * sde);
        auto fill_outputs = [&] {
            fill(proj.p, proj.n * sizeof(float)); fill(dy.p, dy.n * sizeof(float)); fill(coef.p, coef.n * sizeof(float));
            fill(probs.p, probs.n * sizeof(float)); fill(pp.p, pp.n * sizeof(float)); fill(bn_mean.p, bn_mean.n * sizeof(float));
            fill(bn_inv_std.p, bn_inv_std.n * sizeof(float)); fill(acc.p, acc.n * sizeof(double));
        };
        // the workspace of the ordered sum, as Model::alloc_sums sizes it for a largest batch of B; the counters zeroed ONCE
        GridSumWs ws{};
        ws.colgroups = 1; ws.contrib_cap = static_cast<int>((B + 3) / 4); ws.width_cap = 2 * de + 1;
        ws.groups_cap = ws.contrib_cap / 16 + 1; ws.fan = 16;
        part.alloc(static_cast<size_t>(ws.contrib_cap) * ws.width_cap); part2.alloc(static_cast<size_t>(ws.groups_cap) * ws.width_cap);
        arrive.alloc(static_cast<size_t>(ws.groups_cap) + 1, true);
        fill(part.p, part.n * sizeof(double)); fill(part2.p, part2.n * sizeof(double));
        ws.part = part.p; ws.part2 = part2.p; ws.arrive = arrive.p;

        LossArgs l{};
        l.pre = pre.p; l.bn_mean = bn_mean.p; l.bn_inv_std = bn_inv_std.p; l.bias = bias.p;
        l.bn_sums = bn_sums.p; l.bn_n = a->bn_n; l.bn_eps = 1e-4f;
        l.E = E.p; l.E_rows = a->rows_for_dispatch ? a->rows_for_dispatch : rows; l.ids = ids.p; l.inst_w = inst_w.p;
        l.proj = proj.p; l.dy = dy.p; l.coef = coef.p; l.probs = probs.p; l.pp = pp.p;
        l.loss_acc = acc.p; l.colstats = acc.p + 1; l.sums = ws;
        l.B = B; l.de = de; l.R = R;
        l.bn = bn; l.nonlinearity = a->nonlinearity; l.l2_entity = a->l2_entity != 0;
        fill_loss_consts(l, a->clip_sigmoid != 0, a->bias_negative_samples != 0, k, a->b_global);
        if (lazy) { l.lazyE.stamp = stamp.p; l.lazyE.now = a->now; std::memcpy(l.lazyE.decay, a->decay, sizeof(l.lazyE.decay)); }

        LossPlan plan;
        loss_plan(l, &plan);
        if (plan.grid > ws.contrib_cap) throw Error(NVSM_ERR_STATE, "loss: the plan has more workgroups than the workspace has contributions");
        hipStream_t s;
        NVSM_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        try {
            for (int rep = 0; rep < a->repeats; ++rep) {
                fill_outputs();
                NVSM_HIP_CHECK(hipDeviceSynchronize());
                launch_loss(l, s);
                NVSM_HIP_CHECK(hipGetLastError());
                NVSM_HIP_CHECK(hipStreamSynchronize(s));
            }
        } catch (...) {
            (void)hipStreamDestroy(s);
            throw;
        }
        (void)hipStreamDestroy(s);

        down(a->proj, proj.p, proj.n * sizeof(float)); down(a->dy, dy.p, dy.n * sizeof(float));
        down(a->coef, coef.p, coef.n * sizeof(float)); down(a->probs, probs.p, probs.n * sizeof(float));
        down(a->pp, pp.p, pp.n * sizeof(float));
        down(a->bn_mean, bn_mean.p, bn_mean.n * sizeof(float)); down(a->bn_inv_std, bn_inv_std.p, bn_inv_std.n * sizeof(float));
        down(a->loss, acc.p, sizeof(double)); down(a->colstats, acc.p + 1, 3 * sde * sizeof(double));
        if (a->plan) {
            const int out[10] = {plan.family, plan.rb, plan.lazy, plan.pipe, plan.v, plan.niter, plan.l2e, plan.epw, plan.grid, plan.shmem};
            std::memcpy(a->plan, out, sizeof(out));
        }
        if (a->arrive_left) {
            std::vector<int> h(arrive.n);
            down(h.data(), arrive.p, arrive.n * sizeof(int));
            int left = 0;
            for (int v : h) left += v != 0;
            *a->arrive_left = left;
        }
    });
}

int nvsm_debug_gather_mean(int64_t num_rows, int dim, const float* table, const int64_t* idx, const float* wts,
                           int window, int64_t num_out, float* out) {
    NVSM_REQUIRE(table); NVSM_REQUIRE(idx); NVSM_REQUIRE(out);
    return guarded_hook([&] {
        cunvsm::DevBuf<float> T, W, O;
        cunvsm::DevBuf<int64_t> I64;
        cunvsm::DevBuf<int> I;
        T.alloc(num_rows * dim); O.alloc(num_out * dim); I64.alloc(num_out * window); I.alloc(num_out * window);
        NVSM_HIP_CHECK(hipMemcpy(T.p, table, T.n * sizeof(float), hipMemcpyHostToDevice));
        NVSM_HIP_CHECK(hipMemcpy(I64.p, idx, I64.n * sizeof(int64_t), hipMemcpyHostToDevice));
        if (wts) { W.alloc(num_out * window); NVSM_HIP_CHECK(hipMemcpy(W.p, wts, W.n * sizeof(float), hipMemcpyHostToDevice)); }
        cunvsm::launch_narrow_i64(I64.p, I.p, num_out * window, num_rows, nullptr, 0, nullptr);
        cunvsm::launch_gather_mean(T.p, dim, I.p, wts ? W.p : nullptr, window, num_out, O.p, nullptr);
        NVSM_HIP_CHECK(hipDeviceSynchronize());
        NVSM_HIP_CHECK(hipMemcpy(out, O.p, O.n * sizeof(float), hipMemcpyDeviceToHost));
    });
}

int nvsm_debug_gather_mean_lazy(int64_t num_rows, int dim, const float* table, const int64_t* idx, const float* wts,
                                int window, int64_t num_out, const int32_t* stamp, const float* decay, int now,
                                float* out, float* table_out) {
    NVSM_REQUIRE(table); NVSM_REQUIRE(idx); NVSM_REQUIRE(out); NVSM_REQUIRE(stamp); NVSM_REQUIRE(decay); NVSM_REQUIRE(table_out);
    return guarded_hook([&] {
        if (num_rows < 1 || num_rows >= (int64_t(1) << 31) || dim < 1 || window < 1 || num_out < 1) throw Error(NVSM_ERR_INVALID_ARGUMENT, "gather_mean_lazy: bad sizes");
        for (int64_t i = 0; i < num_out * window; ++i)
            if (idx[i] < 0 || idx[i] >= num_rows) throw Error(NVSM_ERR_INVALID_ARGUMENT, "gather_mean_lazy: id out of range");
        require_lags("gather_mean_lazy", stamp, num_rows, now);
        cunvsm::DevBuf<float> T, W, O;
        cunvsm::DevBuf<int64_t> I64;
        cunvsm::DevBuf<int> I, S;
        T.alloc(num_rows * dim); O.alloc(num_out * dim); I64.alloc(num_out * window); I.alloc(num_out * window); S.alloc(num_rows);
        NVSM_HIP_CHECK(hipMemcpy(T.p, table, T.n * sizeof(float), hipMemcpyHostToDevice));
        NVSM_HIP_CHECK(hipMemcpy(I64.p, idx, I64.n * sizeof(int64_t), hipMemcpyHostToDevice));
        NVSM_HIP_CHECK(hipMemcpy(S.p, stamp, S.n * sizeof(int), hipMemcpyHostToDevice));
        NVSM_HIP_CHECK(hipMemset(O.p, 0xFF, O.n * sizeof(float)));
        if (wts) { W.alloc(num_out * window); NVSM_HIP_CHECK(hipMemcpy(W.p, wts, W.n * sizeof(float), hipMemcpyHostToDevice)); }
        cunvsm::LazyView view{};
        view.stamp = S.p; view.now = now; std::memcpy(view.decay, decay, sizeof(view.decay));
        cunvsm::launch_narrow_i64(I64.p, I.p, num_out * window, num_rows, nullptr, 0, nullptr);
        cunvsm::launch_gather_mean(T.p, dim, I.p, wts ? W.p : nullptr, window, num_out, O.p, nullptr, &view);
        NVSM_HIP_CHECK(hipGetLastError());
        NVSM_HIP_CHECK(hipDeviceSynchronize());
        NVSM_HIP_CHECK(hipMemcpy(out, O.p, O.n * sizeof(float), hipMemcpyDeviceToHost));
        NVSM_HIP_CHECK(hipMemcpy(table_out, T.p, T.n * sizeof(float), hipMemcpyDeviceToHost));
    });
}

// One launch_ngram_rows on caller-supplied inputs (cunvsm_amd_test_hooks.h): the caller's buffer goes up whole, guard rows and all,
// the launch writes S rows from out_row0 on, and the buffer comes back whole.
int nvsm_debug_ngram_rows(const float* G, int64_t m, int de, const float* bias, float c, int act, int64_t p0, int64_t S, float* out,
                          int64_t out_rows, int64_t out_row0) {
    NVSM_REQUIRE(G); NVSM_REQUIRE(bias); NVSM_REQUIRE(out);
    return guarded_hook([&] {
        using namespace cunvsm;
        const int64_t rows = m < 65536 ? ngram_row_count(m, 2) : -1;
        if (rows < 0 || de < 1 || S < 1 || S >= (int64_t(1) << 31) || p0 < 0 || p0 + S > rows || out_row0 < 0 || out_row0 + S > out_rows)
            throw Error(NVSM_ERR_INVALID_ARGUMENT, "ngram_rows: bad sizes");
        DevBuf<float> g, b, o;
        g.alloc(static_cast<size_t>(m) * de); b.alloc(static_cast<size_t>(de)); o.alloc(static_cast<size_t>(out_rows) * de);
        NVSM_HIP_CHECK(hipMemcpy(g.p, G, g.n * sizeof(float), hipMemcpyHostToDevice));
        NVSM_HIP_CHECK(hipMemcpy(b.p, bias, b.n * sizeof(float), hipMemcpyHostToDevice));
        NVSM_HIP_CHECK(hipMemcpy(o.p, out, o.n * sizeof(float), hipMemcpyHostToDevice));
        launch_ngram_rows(g.p, static_cast<int>(m), de, b.p, c, act, p0, static_cast<int>(S), o.p + out_row0 * de, nullptr);
        NVSM_HIP_CHECK(hipGetLastError());
        NVSM_HIP_CHECK(hipDeviceSynchronize());
        NVSM_HIP_CHECK(hipMemcpy(out, o.p, o.n * sizeof(float), hipMemcpyDeviceToHost));
    });
}

// ---- nvsm_tsne's stages on caller-supplied inputs (cunvsm_amd_test_hooks.h): the product's launchers and its host functions
// (kernels.h launch_tsne_*, model.h tsne_pca_start / tsne_descent) on a scratch of the hook's own
namespace {
void tsne_hook_sizes(int64_t n, int64_t d) {
    if (n < 2 || n > NVSM_TSNE_MAX_ROWS || d < 1 || d > 4096) throw Error(NVSM_ERR_INVALID_ARGUMENT, "tsne hook: bad sizes");
}
// host [rows][n] <-> device rows of tsne_ld(n) floats
void tsne_hook_up(float* dev, const float* host, int64_t n, int64_t rows) {
    NVSM_HIP_CHECK(hipMemcpy2D(dev, cunvsm::tsne_ld(n) * sizeof(float), host, n * sizeof(float), n * sizeof(float), rows, hipMemcpyHostToDevice));
}
void tsne_hook_down(float* host, const float* dev, int64_t n, int64_t rows) {
    NVSM_HIP_CHECK(hipMemcpy2D(host, n * sizeof(float), dev, cunvsm::tsne_ld(n) * sizeof(float), n * sizeof(float), rows, hipMemcpyDeviceToHost));
}
}  // namespace

int nvsm_debug_tsne_affinities(const float* X, int64_t n, int d, float perplexity, float* P_out, float* cond_out) {
    NVSM_REQUIRE(X); NVSM_REQUIRE(P_out);
    return guarded_hook([&] {
        using namespace cunvsm;
        tsne_hook_sizes(n, d);
        if (!(perplexity > 0.f) || !(perplexity < static_cast<float>(n))) throw Error(NVSM_ERR_INVALID_ARGUMENT, "tsne hook: bad perplexity");
        const int64_t ld = tsne_ld(n);
        DevBuf<float> x, p, c;
        DevBuf<double> w;
        x.alloc(static_cast<size_t>(n) * d); p.alloc(static_cast<size_t>(n + 2) * ld); w.alloc(static_cast<size_t>(n) + 1);
        if (cond_out) c.alloc(static_cast<size_t>(n) * ld);
        NVSM_HIP_CHECK(hipMemcpy(x.p, X, x.n * sizeof(float), hipMemcpyHostToDevice));
        tsne_hook_up(p.p, P_out, n, n + 2);      // the caller's guard rows 0 and n + 1 go up and must come back as they are
        launch_tsne_conditionals(x.p, static_cast<int>(n), d, perplexity, p.p + ld, w.p, nullptr);
        if (cond_out)      // (what the symmetrised P no longer shows)
            NVSM_HIP_CHECK(hipMemcpyAsync(c.p, p.p + ld, static_cast<size_t>(n) * ld * sizeof(float), hipMemcpyDeviceToDevice, nullptr));
        launch_tsne_joint(p.p + ld, static_cast<int>(n), w.p, w.p + n, nullptr);
        NVSM_HIP_CHECK(hipGetLastError());
        NVSM_HIP_CHECK(hipDeviceSynchronize());
        tsne_hook_down(P_out, p.p, n, n + 2);
        if (cond_out) tsne_hook_down(cond_out, c.p, n, n);
    });
}

int nvsm_debug_tsne_gradient(const float* P, const float* Y, int64_t n, float exaggeration, float* grad_out, double* kl_out) {
    NVSM_REQUIRE(P); NVSM_REQUIRE(Y); NVSM_REQUIRE(grad_out); NVSM_REQUIRE(kl_out);
    return guarded_hook([&] {
        using namespace cunvsm;
        tsne_hook_sizes(n, 1);
        TsneScratch w;
        w.grow_for(n, 1);
        DevBuf<float> graw;
        graw.alloc(static_cast<size_t>(2 * n));
        const int rows = static_cast<int>(n);
        double* klrow = w.rows.p + n;
        double* z = w.rows.p + 2 * n + 1;
        tsne_hook_up(w.p.p, P, n, n);
        NVSM_HIP_CHECK(hipMemcpy(w.y.p, Y, static_cast<size_t>(2 * n) * sizeof(float), hipMemcpyHostToDevice));
        NVSM_HIP_CHECK(hipMemset(w.upd.p, 0, static_cast<size_t>(2 * n) * sizeof(float)));
        NVSM_HIP_CHECK(hipMemset(w.gains.p, 0, static_cast<size_t>(2 * n) * sizeof(float)));
        NVSM_HIP_CHECK(hipDeviceSynchronize());
        launch_tsne_forces(w.p.p, w.y.p, rows, w.part.p, z, nullptr);
        launch_tsne_kl_rows(w.p.p, w.y.p, rows, z + 3, exaggeration, klrow, nullptr);
        // a step of learning rate 0 on zero gains and updates: Y stays, graw is the gradient
        launch_tsne_update(w.part.p, rows, z, exaggeration, 0.f, 0.f, w.y.p, w.upd.p, w.gains.p, w.gs.p, graw.p, nullptr);
        launch_tsne_check(klrow, w.gs.p, rows, z + 1, nullptr);
        NVSM_HIP_CHECK(hipGetLastError());
        NVSM_HIP_CHECK(hipDeviceSynchronize());
        NVSM_HIP_CHECK(hipMemcpy(grad_out, graw.p, static_cast<size_t>(2 * n) * sizeof(float), hipMemcpyDeviceToHost));
        NVSM_HIP_CHECK(hipMemcpy(kl_out, z + 1, sizeof(double), hipMemcpyDeviceToHost));
    });
}

int nvsm_debug_tsne_pca(const float* X, int64_t n, int d, float* Y0_out) {
    NVSM_REQUIRE(X); NVSM_REQUIRE(Y0_out);
    return guarded_hook([&] {
        using namespace cunvsm;
        tsne_hook_sizes(n, d);
        TsneScratch w;
        w.grow_for(n, d);
        NVSM_HIP_CHECK(hipMemcpy(w.x.p, X, static_cast<size_t>(n) * d * sizeof(float), hipMemcpyHostToDevice));
        tsne_pca_start(w.x.p, static_cast<int>(n), d, w, w.y.p, nullptr);
        NVSM_HIP_CHECK(hipGetLastError());
        NVSM_HIP_CHECK(hipMemcpy(Y0_out, w.y.p, static_cast<size_t>(2 * n) * sizeof(float), hipMemcpyDeviceToHost));
    });
}

int nvsm_debug_tsne_descent(const float* P, float* Y, int64_t n, const nvsm_tsne_options* opt, int exploration, double* kl_out,
                            int32_t* n_iter_out) {
    NVSM_REQUIRE(P); NVSM_REQUIRE(Y); NVSM_REQUIRE(opt); NVSM_REQUIRE(kl_out); NVSM_REQUIRE(n_iter_out);
    return guarded_hook([&] {
        using namespace cunvsm;
        tsne_hook_sizes(n, 1);
        if (opt->max_iter < 1 || opt->max_iter > 100000 || exploration < 1 || exploration > opt->max_iter || !(opt->learning_rate > 0.f) ||
            !(opt->early_exaggeration > 0.f) || opt->n_iter_without_progress < 0)
            throw Error(NVSM_ERR_INVALID_ARGUMENT, "tsne hook: bad options");
        TsneScratch w;
        w.grow_for(n, 1);
        tsne_hook_up(w.p.p, P, n, n);
        NVSM_HIP_CHECK(hipMemcpy(w.y.p, Y, static_cast<size_t>(2 * n) * sizeof(float), hipMemcpyHostToDevice));
        tsne_descent(w, static_cast<int>(n), *opt, opt->learning_rate, exploration, kl_out, n_iter_out, nullptr, nullptr);
        NVSM_HIP_CHECK(hipGetLastError());
        NVSM_HIP_CHECK(hipMemcpy(Y, w.y.p, static_cast<size_t>(2 * n) * sizeof(float), hipMemcpyDeviceToHost));
    });
}

// ---- nvsm_tsne_sparse's stages on caller-supplied inputs (cunvsm_amd_test_hooks.h): the product's launchers (kernels.h
// launch_tsne_nn_* / launch_tsne_sparse_*) and host functions (model.h tsne_sparse_*) on a scratch of the hook's own
namespace {
constexpr int64_t kTsneHookScoreFloats = int64_t(256) << 18;      // the default score slab of a retrieval round: 256 MB
void tsne_sparse_hook_sizes(int64_t n, int64_t d, int64_t k) {
    if (n < 2 || n > NVSM_TSNE_SPARSE_MAX_ROWS || d < 1 || d > 4096 || k < 1 || k > n - 1 || k > NVSM_TSNE_SPARSE_MAX_NEIGHBORS ||
        2 * n * k >= (int64_t(1) << 31))
        throw Error(NVSM_ERR_INVALID_ARGUMENT, "tsne sparse hook: bad sizes");
}
// the caller's CSR matrix (indptr [n + 1], indices / data [nnz]) into the scratch, checked: the kernels trust what they index with
void tsne_sparse_hook_csr(cunvsm::TsneSparseScratch& w, const int64_t* indptr, const int32_t* indices, const float* data, int64_t n) {
    if (indptr[0] != 0) throw Error(NVSM_ERR_INVALID_ARGUMENT, "tsne sparse hook: indptr[0] must be 0");
    for (int64_t i = 0; i < n; ++i)
        if (indptr[i + 1] < indptr[i]) throw Error(NVSM_ERR_INVALID_ARGUMENT, "tsne sparse hook: indptr decreases");
    const int64_t nnz = indptr[n];
    if (nnz >= (int64_t(1) << 31)) throw Error(NVSM_ERR_INVALID_ARGUMENT, "tsne sparse hook: too many entries");
    for (int64_t p = 0; p < nnz; ++p)
        if (indices[p] < 0 || indices[p] >= n) throw Error(NVSM_ERR_INVALID_ARGUMENT, "tsne sparse hook: a column is outside the matrix");
    w.nnz = nnz;
    w.indices.alloc(static_cast<size_t>(std::max<int64_t>(nnz, 1)));
    w.data.alloc(static_cast<size_t>(std::max<int64_t>(nnz, 1)));
    NVSM_HIP_CHECK(hipMemcpy(w.indptr.p, indptr, static_cast<size_t>(n + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    if (nnz > 0) {
        NVSM_HIP_CHECK(hipMemcpy(w.indices.p, indices, static_cast<size_t>(nnz) * sizeof(int32_t), hipMemcpyHostToDevice));
        NVSM_HIP_CHECK(hipMemcpy(w.data.p, data, static_cast<size_t>(nnz) * sizeof(float), hipMemcpyHostToDevice));
    }
}
}  // namespace

int nvsm_debug_tsne_knn(const float* X, int64_t n, int d, int k, int64_t round_rows, int32_t* ids_out, float* d2_out) {
    NVSM_REQUIRE(X); NVSM_REQUIRE(ids_out); NVSM_REQUIRE(d2_out);
    return guarded_hook([&] {
        using namespace cunvsm;
        tsne_sparse_hook_sizes(n, d, k);
        if (round_rows < 0) throw Error(NVSM_ERR_INVALID_ARGUMENT, "tsne sparse hook: round_rows is negative");
        TsneSparseScratch w;
        w.grow_rows(n, d);
        NVSM_HIP_CHECK(hipMemcpy(w.base.x.p, X, static_cast<size_t>(n) * d * sizeof(float), hipMemcpyHostToDevice));
        tsne_sparse_knn(w.base.x.p, static_cast<int>(n), d, k, round_rows, kTsneHookScoreFloats, w, nullptr, nullptr);
        NVSM_HIP_CHECK(hipGetLastError());
        NVSM_HIP_CHECK(hipDeviceSynchronize());
        NVSM_HIP_CHECK(hipMemcpy(ids_out, w.nbr_id.p, static_cast<size_t>(n) * k * sizeof(int32_t), hipMemcpyDeviceToHost));
        NVSM_HIP_CHECK(hipMemcpy(d2_out, w.nbr_d2.p, static_cast<size_t>(n) * k * sizeof(float), hipMemcpyDeviceToHost));
    });
}

int nvsm_debug_tsne_sparse_affinities(const float* X, int64_t n, int d, float perplexity, int k, int64_t* indptr_out, int32_t* indices_out,
                                      float* data_out, float* cond_out) {
    NVSM_REQUIRE(X); NVSM_REQUIRE(indptr_out); NVSM_REQUIRE(indices_out); NVSM_REQUIRE(data_out);
    return guarded_hook([&] {
        using namespace cunvsm;
        tsne_sparse_hook_sizes(n, d, k);
        if (!(perplexity > 0.f) || !(perplexity < static_cast<float>(n))) throw Error(NVSM_ERR_INVALID_ARGUMENT, "tsne sparse hook: bad perplexity");
        TsneSparseScratch w;
        w.grow_rows(n, d);
        NVSM_HIP_CHECK(hipMemcpy(w.base.x.p, X, static_cast<size_t>(n) * d * sizeof(float), hipMemcpyHostToDevice));
        tsne_sparse_knn(w.base.x.p, static_cast<int>(n), d, k, 0, kTsneHookScoreFloats, w, nullptr, nullptr);
        tsne_sparse_affinities(static_cast<int>(n), k, perplexity, w, nullptr, nullptr);
        NVSM_HIP_CHECK(hipGetLastError());
        NVSM_HIP_CHECK(hipDeviceSynchronize());
        NVSM_HIP_CHECK(hipMemcpy(indptr_out, w.indptr.p, static_cast<size_t>(n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
        NVSM_HIP_CHECK(hipMemcpy(indices_out, w.indices.p, static_cast<size_t>(w.nnz) * sizeof(int32_t), hipMemcpyDeviceToHost));
        NVSM_HIP_CHECK(hipMemcpy(data_out, w.data.p, static_cast<size_t>(w.nnz) * sizeof(float), hipMemcpyDeviceToHost));
        if (cond_out) NVSM_HIP_CHECK(hipMemcpy(cond_out, w.cond.p, static_cast<size_t>(n) * k * sizeof(float), hipMemcpyDeviceToHost));
    });
}

int nvsm_debug_tsne_sparse_gradient(const int64_t* indptr, const int32_t* indices, const float* data, const float* Y, int64_t n,
                                    float exaggeration, int ranges, float* grad_out, double* kl_out) {
    NVSM_REQUIRE(indptr); NVSM_REQUIRE(indices); NVSM_REQUIRE(data); NVSM_REQUIRE(Y); NVSM_REQUIRE(grad_out); NVSM_REQUIRE(kl_out);
    return guarded_hook([&] {
        using namespace cunvsm;
        tsne_sparse_hook_sizes(n, 1, 1);
        if (ranges < 0 || ranges > 4096) throw Error(NVSM_ERR_INVALID_ARGUMENT, "tsne sparse hook: bad ranges");
        TsneSparseScratch w;
        w.forced_ranges = ranges;
        w.grow_rows(n, 1);
        tsne_sparse_hook_csr(w, indptr, indices, data, n);
        TsneScratch& b = w.base;
        DevBuf<float> graw;
        graw.alloc(static_cast<size_t>(2 * n));
        const int rows = static_cast<int>(n);
        double* klrow = b.rows.p + n;
        double* z = b.rows.p + 2 * n + 1;
        NVSM_HIP_CHECK(hipMemcpy(b.y.p, Y, static_cast<size_t>(2 * n) * sizeof(float), hipMemcpyHostToDevice));
        NVSM_HIP_CHECK(hipMemset(b.upd.p, 0, static_cast<size_t>(2 * n) * sizeof(float)));
        NVSM_HIP_CHECK(hipMemset(b.gains.p, 0, static_cast<size_t>(2 * n) * sizeof(float)));
        NVSM_HIP_CHECK(hipDeviceSynchronize());
        launch_tsne_sparse_forces(w.indptr.p, w.indices.p, w.data.p, b.y.p, rows, ranges, w.attr.p, w.part.p, z, nullptr);
        launch_tsne_sparse_kl_rows(w.indptr.p, w.indices.p, w.data.p, b.y.p, rows, z + 3, exaggeration, klrow, nullptr);
        // a step of learning rate 0 on zero gains and updates: Y stays, graw is the gradient
        launch_tsne_sparse_update(w.attr.p, w.part.p, rows, ranges, z, exaggeration, 0.f, 0.f, b.y.p, b.upd.p, b.gains.p, b.gs.p, graw.p, nullptr);
        launch_tsne_check(klrow, b.gs.p, rows, z + 1, nullptr);
        NVSM_HIP_CHECK(hipGetLastError());
        NVSM_HIP_CHECK(hipDeviceSynchronize());
        NVSM_HIP_CHECK(hipMemcpy(grad_out, graw.p, static_cast<size_t>(2 * n) * sizeof(float), hipMemcpyDeviceToHost));
        NVSM_HIP_CHECK(hipMemcpy(kl_out, z + 1, sizeof(double), hipMemcpyDeviceToHost));
    });
}

int nvsm_debug_tsne_sparse_descent(const int64_t* indptr, const int32_t* indices, const float* data, float* Y, int64_t n,
                                   const nvsm_tsne_options* opt, int exploration, double* kl_out, int32_t* n_iter_out) {
    NVSM_REQUIRE(indptr); NVSM_REQUIRE(indices); NVSM_REQUIRE(data); NVSM_REQUIRE(Y); NVSM_REQUIRE(opt); NVSM_REQUIRE(kl_out);
    NVSM_REQUIRE(n_iter_out);
    return guarded_hook([&] {
        using namespace cunvsm;
        tsne_sparse_hook_sizes(n, 1, 1);
        if (opt->max_iter < 1 || opt->max_iter > 100000 || exploration < 1 || exploration > opt->max_iter || !(opt->learning_rate > 0.f) ||
            !(opt->early_exaggeration > 0.f) || opt->n_iter_without_progress < 0)
            throw Error(NVSM_ERR_INVALID_ARGUMENT, "tsne sparse hook: bad options");
        TsneSparseScratch w;
        w.grow_rows(n, 1);
        tsne_sparse_hook_csr(w, indptr, indices, data, n);
        NVSM_HIP_CHECK(hipMemcpy(w.base.y.p, Y, static_cast<size_t>(2 * n) * sizeof(float), hipMemcpyHostToDevice));
        tsne_sparse_descent(w, static_cast<int>(n), *opt, opt->learning_rate, exploration, kl_out, n_iter_out, nullptr, nullptr);
        NVSM_HIP_CHECK(hipGetLastError());
        NVSM_HIP_CHECK(hipMemcpy(Y, w.base.y.p, static_cast<size_t>(2 * n) * sizeof(float), hipMemcpyDeviceToHost));
    });
}

// ---- nvsm_kmeans' passes on caller-supplied inputs (cunvsm_amd_test_hooks.h): the product's launchers and host functions
// (kernels.h launch_kmeans_*, model.h kmeans_*) on a scratch of the hook's own
namespace {
void kmeans_hook_sizes(int64_t n, int64_t d, int64_t k) {
    if (n < 1 || n >= (int64_t(1) << 31) || d < 1 || d > 4096 || k < 1 || k > n || k > NVSM_KMEANS_MAX_CLUSTERS)
        throw Error(NVSM_ERR_INVALID_ARGUMENT, "kmeans hook: bad sizes");
}
}  // namespace

int nvsm_debug_kmeans_assign(const float* X, int64_t n, int d, const float* C, int k, int32_t* labels_out, float* dist_out) {
    NVSM_REQUIRE(X); NVSM_REQUIRE(C); NVSM_REQUIRE(labels_out);
    return guarded_hook([&] {
        using namespace cunvsm;
        kmeans_hook_sizes(n, d, k);
        KmeansScratch w;
        w.grow_for(n, d, k);
        NVSM_HIP_CHECK(hipMemcpy(w.x.p, X, static_cast<size_t>(n) * d * sizeof(float), hipMemcpyHostToDevice));
        NVSM_HIP_CHECK(hipMemcpy(w.c.p, C, static_cast<size_t>(k) * d * sizeof(float), hipMemcpyHostToDevice));
        kmeans_prepare(w, static_cast<int>(n), d, nullptr);
        kmeans_assign_pass(w, static_cast<int>(n), d, k, w.c.p, w.lab_a.p, nullptr);
        NVSM_HIP_CHECK(hipGetLastError());
        NVSM_HIP_CHECK(hipDeviceSynchronize());
        NVSM_HIP_CHECK(hipMemcpy(labels_out, w.lab_a.p, static_cast<size_t>(n) * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (dist_out) NVSM_HIP_CHECK(hipMemcpy(dist_out, w.dist32.p, static_cast<size_t>(n) * sizeof(float), hipMemcpyDeviceToHost));
    });
}

int nvsm_debug_kmeans_update(const float* X, int64_t n, int d, int32_t* labels, const float* C_old, int k, float* C_new,
                             int64_t* counts_out, double* shift_out) {
    NVSM_REQUIRE(X); NVSM_REQUIRE(labels); NVSM_REQUIRE(C_old); NVSM_REQUIRE(C_new); NVSM_REQUIRE(counts_out); NVSM_REQUIRE(shift_out);
    return guarded_hook([&] {
        using namespace cunvsm;
        kmeans_hook_sizes(n, d, k);
        for (int64_t i = 0; i < n; ++i)
            if (labels[i] < 0 || labels[i] >= k) throw Error(NVSM_ERR_INVALID_ARGUMENT, "kmeans hook: a label is outside [0, k)");
        KmeansScratch w;
        w.grow_for(n, d, k);
        NVSM_HIP_CHECK(hipMemcpy(w.x.p, X, static_cast<size_t>(n) * d * sizeof(float), hipMemcpyHostToDevice));
        NVSM_HIP_CHECK(hipMemcpy(w.c.p, C_old, static_cast<size_t>(k) * d * sizeof(float), hipMemcpyHostToDevice));
        NVSM_HIP_CHECK(hipMemcpy(w.lab_a.p, labels, static_cast<size_t>(n) * sizeof(int32_t), hipMemcpyHostToDevice));
        kmeans_update_pass(w, static_cast<int>(n), d, k, w.lab_a.p, w.c.p, w.c2.p, true, nullptr);
        NVSM_HIP_CHECK(hipGetLastError());
        NVSM_HIP_CHECK(hipDeviceSynchronize());
        NVSM_HIP_CHECK(hipMemcpy(labels, w.lab_a.p, static_cast<size_t>(n) * sizeof(int32_t), hipMemcpyDeviceToHost));
        NVSM_HIP_CHECK(hipMemcpy(C_new, w.c2.p, static_cast<size_t>(k) * d * sizeof(float), hipMemcpyDeviceToHost));
        NVSM_HIP_CHECK(hipMemcpy(counts_out, w.counts.p, static_cast<size_t>(k) * sizeof(int64_t), hipMemcpyDeviceToHost));
        NVSM_HIP_CHECK(hipMemcpy(shift_out, w.scalars(static_cast<int>(n), d) + 1, sizeof(double), hipMemcpyDeviceToHost));
    });
}

int nvsm_debug_kmeans_plusplus(const float* X, int64_t n, int d, int k, int64_t seed, int64_t* rows_out, float* centers_out) {
    NVSM_REQUIRE(X); NVSM_REQUIRE(rows_out);
    return guarded_hook([&] {
        using namespace cunvsm;
        kmeans_hook_sizes(n, d, k);
        if (seed < 1) throw Error(NVSM_ERR_INVALID_ARGUMENT, "kmeans hook: seed must be at least 1");
        KmeansScratch w;
        w.grow_for(n, d, k);
        NVSM_HIP_CHECK(hipMemcpy(w.x.p, X, static_cast<size_t>(n) * d * sizeof(float), hipMemcpyHostToDevice));
        kmeans_plusplus(w, static_cast<int>(n), d, k, seed, w.c.p, rows_out, nullptr);
        NVSM_HIP_CHECK(hipGetLastError());
        if (centers_out) NVSM_HIP_CHECK(hipMemcpy(centers_out, w.c.p, static_cast<size_t>(k) * d * sizeof(float), hipMemcpyDeviceToHost));
    });
}

// One launch_lazy_refresh on caller-supplied inputs (cunvsm_amd_test_hooks.h): the arguments of Model::lazy_refresh /
// Model::lazy_scalar_snapshot, the list and its count on the device as Csr::touched / num_touched are.
int nvsm_debug_lazy_refresh(const nvsm_debug_lazy_refresh_args* a) {
    NVSM_REQUIRE(a); NVSM_REQUIRE(a->P); NVSM_REQUIRE(a->stamp); NVSM_REQUIRE(a->stamp_out); NVSM_REQUIRE(a->decay);
    return guarded_hook([&] {
        using namespace cunvsm;
        const int64_t rows = a->rows, nl = a->list ? a->n_list : 0;
        const int dim = a->dim;
        auto bad = [](const char* what) { throw Error(NVSM_ERR_INVALID_ARGUMENT, std::string("lazy_refresh: ") + what); };
        if (rows < 1 || rows >= (int64_t(1) << 30) || dim < 1 || nl < 0 || nl > rows) bad("bad sizes");
        if (a->sc_snapshot && !a->sc) bad("a snapshot needs the scalar");
        std::vector<char> seen(a->list ? static_cast<size_t>(rows) : 0, 0);
        for (int64_t i = 0; i < nl; ++i) {
            if (a->list[i] < 0 || a->list[i] >= rows || seen[a->list[i]]) bad("list: row ids in [0, rows), none twice");
            seen[a->list[i]] = 1;
        }
        require_lags("lazy_refresh", a->stamp, rows, a->now);
        auto up = [](void* d, const void* h, size_t bytes) { if (bytes) NVSM_HIP_CHECK(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice)); };
        auto down = [](void* h, const void* d, size_t bytes) { if (bytes) NVSM_HIP_CHECK(hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost)); };
        const size_t RD = static_cast<size_t>(rows + 1) * dim, R1 = static_cast<size_t>(rows) + 1;
        DevBuf<float> P, m, sc, snap;
        DevBuf<int> stamp, list, count;
        P.alloc(RD); up(P.p, a->P, RD * sizeof(float));
        if (a->m) { m.alloc(RD); up(m.p, a->m, RD * sizeof(float)); }
        if (a->sc) { sc.alloc(R1); up(sc.p, a->sc, R1 * sizeof(float)); }
        if (a->sc_snapshot) { snap.alloc(R1); NVSM_HIP_CHECK(hipMemset(snap.p, 0xFF, R1 * sizeof(float))); }
        stamp.alloc(rows); up(stamp.p, a->stamp, rows * sizeof(int));
        if (a->list) {
            list.alloc(std::max<int64_t>(nl, 1)); up(list.p, a->list, nl * sizeof(int));
            const int n32 = static_cast<int>(nl);
            count.alloc(1); up(count.p, &n32, sizeof(int));
        }
        LazyRefreshArgs r{};
        r.P = P.p; r.m = m.p; r.sc = sc.p; r.sc_snapshot = snap.p; r.scalars_only = a->scalars_only != 0;
        r.stamp = stamp.p; r.list = list.p; r.list_count = count.p;
        r.rows = rows; r.dim = dim; r.now = a->now; r.s_m = a->s_m; r.s_v = a->s_v;
        std::memcpy(r.decay, a->decay, sizeof(r.decay));
        NVSM_HIP_CHECK(hipDeviceSynchronize());
        launch_lazy_refresh(r, a->list ? nl : rows, nullptr);
        NVSM_HIP_CHECK(hipGetLastError());
        NVSM_HIP_CHECK(hipDeviceSynchronize());
        down(a->P, P.p, RD * sizeof(float));
        if (a->m) down(a->m, m.p, RD * sizeof(float));
        if (a->sc) down(a->sc, sc.p, R1 * sizeof(float));
        if (a->sc_snapshot) down(a->sc_snapshot, snap.p, R1 * sizeof(float));
        down(a->stamp_out, stamp.p, rows * sizeof(int));
    });
}

// launch_lex_df on a caller-supplied corpus at a caller-chosen slab (cunvsm_amd_test_hooks.h): what Model::corpus_df runs, with a bit
// table of the hook's own. The corpus is checked on the host: the kernel indexes df and the bit table by token.
int nvsm_debug_lex_df(const int32_t* tokens, int64_t num_tokens, const int64_t* doc_offsets, int64_t num_documents, int64_t num_words,
                      int64_t slab, int64_t* df_out) {
    NVSM_REQUIRE(doc_offsets); NVSM_REQUIRE(df_out);
    if (num_tokens > 0) NVSM_REQUIRE(tokens);
    return guarded_hook([&] {
        using namespace cunvsm;
        auto bad = [](const char* what) { throw Error(NVSM_ERR_INVALID_ARGUMENT, std::string("lex_df: ") + what); };
        if (num_tokens < 0 || num_documents < 0 || num_documents >= (int64_t(1) << 31) || num_words < 1 || slab < 1 || slab >= (int64_t(1) << 31))
            bad("bad sizes");
        if (lex_df_row_words(slab) > (int64_t(1) << 28) / num_words) bad("the bit table would exceed 1 GiB");
        if (doc_offsets[0] != 0) bad("doc_offsets must start at 0");
        for (int64_t d = 0; d < num_documents; ++d)
            if (doc_offsets[d + 1] < doc_offsets[d]) bad("doc_offsets must not decrease");
        if (doc_offsets[num_documents] != num_tokens) bad("the last of doc_offsets must be num_tokens");
        for (int64_t i = 0; i < num_tokens; ++i)
            if (tokens[i] < 0 || tokens[i] >= num_words) bad("a token is outside [0, num_words)");
        DevBuf<int> tok;
        DevBuf<int64_t> off;
        DevBuf<unsigned long long> df;
        DevBuf<unsigned> bits;
        tok.alloc(static_cast<size_t>(std::max<int64_t>(num_tokens, 1)), true);
        off.alloc(static_cast<size_t>(num_documents) + 1);
        df.alloc(static_cast<size_t>(num_words), true);
        bits.alloc(static_cast<size_t>(num_words * lex_df_row_words(slab)), true);
        if (num_tokens > 0) NVSM_HIP_CHECK(hipMemcpy(tok.p, tokens, static_cast<size_t>(num_tokens) * sizeof(int), hipMemcpyHostToDevice));
        NVSM_HIP_CHECK(hipMemcpy(off.p, doc_offsets, (static_cast<size_t>(num_documents) + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
        NVSM_HIP_CHECK(hipDeviceSynchronize());
        launch_lex_df(tok.p, off.p, num_documents, slab, bits.p, df.p, nullptr);
        NVSM_HIP_CHECK(hipGetLastError());
        NVSM_HIP_CHECK(hipDeviceSynchronize());
        NVSM_HIP_CHECK(hipMemcpy(df_out, df.p, static_cast<size_t>(num_words) * sizeof(int64_t), hipMemcpyDeviceToHost));
    });
}

}  // extern "C"

// ---- the streaming kernels of a training step, one launcher each (cunvsm_amd_test_hooks.h) ----
namespace {
void step_bad(const char* who, const char* what) { throw Error(NVSM_ERR_INVALID_ARGUMENT, std::string(who) + ": " + what); }
void step_fill(void* p, size_t bytes) { if (bytes) NVSM_HIP_CHECK(hipMemset(p, 0xFF, bytes)); }
void step_up(void* d, const void* h, size_t bytes) { if (bytes) NVSM_HIP_CHECK(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice)); }
void step_down(void* h, const void* d, size_t bytes) { if (h && bytes) NVSM_HIP_CHECK(hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost)); }
// a device copy of n host floats
void step_in(cunvsm::DevBuf<float>& d, const float* h, size_t n) { d.alloc(n); step_up(d.p, h, n * sizeof(float)); }
// an output of n owned floats and `guard` more, all 0xFF
void step_out(cunvsm::DevBuf<float>& d, size_t n, size_t guard) { d.alloc(n + guard); step_fill(d.p, (n + guard) * sizeof(float)); }
void step_ids(const char* who, const int32_t* ids, int64_t n, int64_t limit) {
    for (int64_t i = 0; i < n; ++i) if (ids[i] < 0 || ids[i] >= limit) step_bad(who, "id out of range");
}
// the work items of the kernels that count them in 32 bits (adam_u, bn_dx): rows * nvec
void step_items32(const char* who, int64_t rows, int dim) {
    const int64_t nvec = dim % 4 == 0 ? dim / 4 : dim;
    if (rows > ((int64_t(1) << 32) - 1) / nvec) step_bad(who, "rows * vectors per row must stay below 2^32");
}
void step_sync() {
    NVSM_HIP_CHECK(hipGetLastError());
    NVSM_HIP_CHECK(hipDeviceSynchronize());
}
}  // namespace

extern "C" {

int nvsm_debug_adam_u(int64_t rows, int dim, const float* m, const float* v, const int32_t* idx, int window, int64_t B, float bc,
                      float eps, float* U_out) {
    NVSM_REQUIRE(m); NVSM_REQUIRE(v); NVSM_REQUIRE(idx); NVSM_REQUIRE(U_out);
    return guarded_hook([&] {
        using namespace cunvsm;
        if (rows < 1 || rows >= (int64_t(1) << 31) || dim < 1 || window < 1 || B < 1 || B > (int64_t(1) << 40) / window) step_bad("adam_u", "bad sizes");
        step_items32("adam_u", B, dim);
        step_ids("adam_u", idx, B * window, rows);
        DevBuf<float> M, V, U;
        DevBuf<int> I;
        step_in(M, m, static_cast<size_t>(rows) * dim); step_in(V, v, static_cast<size_t>(rows));
        I.alloc(static_cast<size_t>(B) * window); step_up(I.p, idx, I.n * sizeof(int));
        step_out(U, static_cast<size_t>(B) * dim, dim);
        NVSM_HIP_CHECK(hipDeviceSynchronize());
        launch_adam_u(M.p, V.p, dim, I.p, window, B, bc, eps, U.p, nullptr);
        step_sync();
        step_down(U_out, U.p, U.n * sizeof(float));
    });
}

int nvsm_debug_adagrad_scale(int64_t rows, const float* acc, const int32_t* idx, int window, int64_t B, float eps, float* scale_out) {
    NVSM_REQUIRE(acc); NVSM_REQUIRE(idx); NVSM_REQUIRE(scale_out);
    return guarded_hook([&] {
        using namespace cunvsm;
        if (rows < 1 || rows >= (int64_t(1) << 31) || window < 1 || B < 1 || B > (int64_t(1) << 40) / window) step_bad("adagrad_scale", "bad sizes");
        step_ids("adagrad_scale", idx, B * window, rows);
        DevBuf<float> A, S;
        DevBuf<int> I;
        step_in(A, acc, static_cast<size_t>(rows));
        I.alloc(static_cast<size_t>(B) * window); step_up(I.p, idx, I.n * sizeof(int));
        step_out(S, static_cast<size_t>(B), 1);
        NVSM_HIP_CHECK(hipDeviceSynchronize());
        launch_adagrad_scale(A.p, I.p, window, B, eps, S.p, nullptr);
        step_sync();
        step_down(scale_out, S.p, S.n * sizeof(float));
    });
}

int nvsm_debug_bn_dx(const nvsm_debug_bn_dx_args* a) {
    NVSM_REQUIRE(a); NVSM_REQUIRE(a->sums); NVSM_REQUIRE(a->grad_bias);
    return guarded_hook([&] {
        using namespace cunvsm;
        const int64_t rows = a->rows;
        const int dim = a->dim;
        const size_t sd = static_cast<size_t>(dim > 0 ? dim : 0);
        if (dim < 1 || dim > (1 << 20)) step_bad("bn_dx", "bad sizes");
        DevBuf<float> dy, pre, mean, inv_std, dbeta, dgamma, gbias;
        DevBuf<double> sums;
        sums.alloc(2 * sd); step_up(sums.p, a->sums, 2 * sd * sizeof(double));
        step_out(dbeta, sd, 1); step_out(dgamma, sd, 1); step_out(gbias, sd, 1);
        if (a->pre) {
            if (rows < 1 || rows >= (int64_t(1) << 31) || !a->dy || !a->mean || !a->inv_std || !a->dy_out || !a->dbeta || !a->dgamma || !(a->n_global > 0))
                step_bad("bn_dx", "the batch-norm backward needs rows, dy, pre, mean, inv_std, n_global > 0 and every output");
            step_items32("bn_dx", rows, dim);
            const size_t RD = static_cast<size_t>(rows) * dim;
            step_out(dy, RD, sd); step_up(dy.p, a->dy, RD * sizeof(float));
            step_in(pre, a->pre, RD); step_in(mean, a->mean, sd); step_in(inv_std, a->inv_std, sd);
            NVSM_HIP_CHECK(hipDeviceSynchronize());
            launch_bn_dx(dy.p, pre.p, mean.p, inv_std.p, sums.p, dbeta.p, dgamma.p, gbias.p, a->n_global, rows, dim, nullptr);
            step_sync();
            step_down(a->dy_out, dy.p, dy.n * sizeof(float));
        } else {
            NVSM_HIP_CHECK(hipDeviceSynchronize());
            launch_colsum_finalize(sums.p, dim, gbias.p, nullptr);
            step_sync();
        }
        step_down(a->dbeta, dbeta.p, dbeta.n * sizeof(float));
        step_down(a->dgamma, dgamma.p, dgamma.n * sizeof(float));
        step_down(a->grad_bias, gbias.p, gbias.n * sizeof(float));
    });
}

int nvsm_debug_row_op(const nvsm_debug_row_op_args* a) {
    NVSM_REQUIRE(a); NVSM_REQUIRE(a->x);
    return guarded_hook([&] {
        using namespace cunvsm;
        const int64_t rows = a->rows;
        const int dim = a->dim, op = a->op;
        if (op < NVSM_DEBUG_ROW_MEANSQ || op > NVSM_DEBUG_ROW_MATERIALIZE_L2) step_bad("row_op", "op 0 .. 4");
        if (rows < 1 || rows >= (int64_t(1) << 24) || dim < 1 || dim > (1 << 16)) step_bad("row_op", "bad sizes");
        const size_t RD = static_cast<size_t>(rows) * dim, sd = static_cast<size_t>(dim), R1 = static_cast<size_t>(rows);
        DevBuf<float> x, g, norms, coef, E, out, sc;
        DevBuf<int> ids;
        const bool wants_out = op != NVSM_DEBUG_ROW_MEANSQ;
        const bool wants_sc = op == NVSM_DEBUG_ROW_MEANSQ || op == NVSM_DEBUG_ROW_L2_FORWARD || a->out_scalar != nullptr;
        if (wants_out && !a->out) step_bad("row_op", "out is required");
        if (op == NVSM_DEBUG_ROW_MATERIALIZE && a->out_scalar) step_bad("row_op", "the plain materialise has no scalar output");
        if (wants_sc && !a->out_scalar) step_bad("row_op", "out_scalar is required");
        if (wants_out) step_out(out, RD, sd);
        if (wants_sc) step_out(sc, R1, 1);
        switch (op) {
        case NVSM_DEBUG_ROW_MEANSQ:
            step_in(x, a->x, RD);
            NVSM_HIP_CHECK(hipDeviceSynchronize());
            launch_row_meansq(x.p, rows, dim, a->scale, sc.p, nullptr);
            break;
        case NVSM_DEBUG_ROW_L2_FORWARD:
            step_in(x, a->x, RD);
            NVSM_HIP_CHECK(hipDeviceSynchronize());
            launch_l2_rows_forward(x.p, rows, dim, out.p, sc.p, nullptr);
            break;
        case NVSM_DEBUG_ROW_L2_BACKWARD:
            if (!a->g || !a->norms) step_bad("row_op", "the normaliser's backward needs g and norms");
            step_in(x, a->x, RD); step_in(norms, a->norms, R1);
            if (a->in_place) step_up(out.p, a->g, RD * sizeof(float));      // (the guard row behind it stays 0xFF)
            else step_in(g, a->g, RD);
            NVSM_HIP_CHECK(hipDeviceSynchronize());
            launch_l2_rows_backward(a->in_place ? out.p : g.p, x.p, norms.p, rows, dim, a->scale, out.p, sc.p, nullptr);
            break;
        default: {
            const int R = a->R;
            if (R < 1 || !a->coef) step_bad("row_op", "the materialise ops need coef and R >= 1");
            const size_t prows = static_cast<size_t>((rows + R - 1) / R);
            step_in(x, a->x, prows * sd); step_in(coef, a->coef, R1);
            if (op == NVSM_DEBUG_ROW_MATERIALIZE_L2) {
                if (!a->E || !a->ids || a->table_rows < 1 || a->table_rows >= (int64_t(1) << 31)) step_bad("row_op", "the normalised materialise needs E, ids and table_rows");
                step_ids("row_op", a->ids, rows, a->table_rows);
                step_in(E, a->E, static_cast<size_t>(a->table_rows) * sd);
                ids.alloc(R1); step_up(ids.p, a->ids, R1 * sizeof(int));
                NVSM_HIP_CHECK(hipDeviceSynchronize());
                launch_materialize_grad_entity_l2(coef.p, x.p, E.p, ids.p, rows, R, dim, out.p, sc.p, nullptr);
            } else {
                NVSM_HIP_CHECK(hipDeviceSynchronize());
                launch_materialize_grad_entity(coef.p, x.p, rows, R, dim, out.p, nullptr);
            }
        }
        }
        step_sync();
        if (wants_out) step_down(a->out, out.p, out.n * sizeof(float));
        if (wants_sc) step_down(a->out_scalar, sc.p, sc.n * sizeof(float));
    });
}

int nvsm_debug_slab_sum(int which, const float* parts, int nparts, int64_t stride, int64_t n, float* out) {
    NVSM_REQUIRE(parts); NVSM_REQUIRE(out);
    return guarded_hook([&] {
        using namespace cunvsm;
        if ((which != 0 && which != 1) || nparts < 1 || nparts > 4096 || n < 1 || stride < n || stride > (int64_t(1) << 32) / nparts)
            step_bad("slab_sum", "which 0 / 1, 1 <= nparts <= 4096, 1 <= n <= stride");
        DevBuf<float> P, O;
        step_in(P, parts, static_cast<size_t>(nparts) * stride);
        step_out(O, static_cast<size_t>(n), 1);
        NVSM_HIP_CHECK(hipDeviceSynchronize());
        if (which == 0) launch_splitk_reduce(P.p, nparts, static_cast<size_t>(stride), O.p, n, nullptr);
        else launch_sum_parts(P.p, nparts, stride, O.p, n, nullptr);
        step_sync();
        step_down(out, O.p, O.n * sizeof(float));
    });
}

int nvsm_debug_plane_sizes(int kind, int N, int K, int64_t* bytes, int64_t* plane_stride) {
    NVSM_REQUIRE(bytes); NVSM_REQUIRE(plane_stride);
    return guarded_hook([&] {
        using namespace cunvsm;
        if ((kind != 1 && kind != 2) || N < 1 || K < 1 || N > (1 << 14) || K > (1 << 14)) step_bad("plane_sizes", "kind 1 / 2, 1 <= N, K <= 16384");
        *bytes = static_cast<int64_t>(kind == 1 ? gemm_split_planes_bytes(N, K) : gemm_rsplit_planes_bytes(N, K));
        const PlaneTarget t = kind == 1 ? gemm_split_plane_target(N, K, nullptr, 0) : gemm_rsplit_plane_target(N, K, nullptr, 0);
        *plane_stride = static_cast<int64_t>(t.plane_stride);
    });
}

int nvsm_debug_transform_update(const nvsm_debug_transform_update_args* a) {
    NVSM_REQUIRE(a); NVSM_REQUIRE(a->T); NVSM_REQUIRE(a->b); NVSM_REQUIRE(a->gT); NVSM_REQUIRE(a->gb);
    return guarded_hook([&] {
        using namespace cunvsm;
        const int dw = a->dw, de = a->de, method = a->method;
        if (method != NVSM_SGD && method != NVSM_ADAGRAD && method != NVSM_ADAM) step_bad("transform_update", "method 0 SGD / 1 Adagrad / 2 Adam");
        if (dw < 1 || de < 1 || dw > (1 << 12) || de > (1 << 12) || a->t_transform < 1) step_bad("transform_update", "bad sizes");
        if (method != NVSM_SGD && (!a->s0T || !a->s0b)) step_bad("transform_update", "Adagrad and Adam need s0T and s0b");
        if (method == NVSM_ADAM && (!a->s1T || !a->s1b)) step_bad("transform_update", "Adam needs s1T and s1b");
        if (a->partial && (a->slabs < 1 || a->slabs > 4096)) step_bad("transform_update", "1 <= slabs <= 4096");
        for (int i = 0; i < 2; ++i) {
            if (a->plane_kind[i] < 0 || a->plane_kind[i] > 2) step_bad("transform_update", "plane_kind 0 / 1 / 2");
            if (a->plane_kind[i] && (!a->planes[i] || !a->fresh[i])) step_bad("transform_update", "a plane target needs planes and fresh");
        }
        const size_t nT = static_cast<size_t>(dw) * de, nb = static_cast<size_t>(de);
        DevBuf<float> T, b, gT, gb, s0T, s0b, s1T, s1b, partial;
        auto inout = [](DevBuf<float>& d, const float* h, size_t n) { step_out(d, n, 1); step_up(d.p, h, n * sizeof(float)); };
        inout(T, a->T, nT); inout(b, a->b, nb); inout(gT, a->gT, nT); inout(gb, a->gb, nb);
        if (a->s0T) { inout(s0T, a->s0T, nT); inout(s0b, a->s0b, nb); }
        if (a->s1T) { inout(s1T, a->s1T, nT); inout(s1b, a->s1b, nb); }
        if (a->partial) step_in(partial, a->partial, static_cast<size_t>(a->slabs) * nT);

        TransformUpdateArgs u{};
        u.T = T.p; u.b = b.p; u.gT = gT.p; u.gb = gb.p;
        u.s0T = s0T.p; u.s0b = s0b.p; u.s1T = s1T.p; u.s1b = s1b.p;
        u.nT = static_cast<int>(nT); u.nb = de; u.de = de;
        fill_transform_consts(u, method, a->lr, a->lambda, a->t_transform);
        if (a->partial) { u.partial = partial.p; u.slabs = a->slabs; u.slab_stride = nT; }
        // pt[0]: the forward product's B (N = de, K = dw), pt[1]: the backward one's (N = dw, K = de, transposed) - Model::update_transform
        DevBuf<char> planes[2], fresh[2];
        for (int i = 0; i < 2; ++i) {
            const int kind = a->plane_kind[i], N = i == 0 ? de : dw, K = i == 0 ? dw : de;
            if (!kind) continue;
            const size_t bytes = kind == 1 ? gemm_split_planes_bytes(N, K) : gemm_rsplit_planes_bytes(N, K);
            planes[i].alloc(bytes, true);                   // zero-filled, as Model's are
            fresh[i].alloc(bytes); step_fill(fresh[i].p, bytes);
            u.pt[i] = kind == 1 ? gemm_split_plane_target(N, K, planes[i].p, i) : gemm_rsplit_plane_target(N, K, planes[i].p, i);
        }
        NVSM_HIP_CHECK(hipDeviceSynchronize());
        launch_transform_update(u, nullptr);
        step_sync();
        for (int i = 0; i < 2; ++i) {      // Model::cut_transform_planes' arguments
            const int kind = a->plane_kind[i];
            if (!kind) continue;
            if (kind == 1) { if (i == 0) launch_gemm_split_planes(0, T.p, de, dw, de, fresh[i].p, nullptr); else launch_gemm_split_planes(1, T.p, dw, de, de, fresh[i].p, nullptr); }
            else { if (i == 0) launch_gemm_rsplit_planes(0, T.p, de, dw, de, fresh[i].p, nullptr); else launch_gemm_rsplit_planes(1, T.p, dw, de, de, fresh[i].p, nullptr); }
        }
        step_sync();
        step_down(a->T, T.p, T.n * sizeof(float)); step_down(a->b, b.p, b.n * sizeof(float));
        step_down(a->gT, gT.p, gT.n * sizeof(float)); step_down(a->gb, gb.p, gb.n * sizeof(float));
        if (a->s0T) { step_down(a->s0T, s0T.p, s0T.n * sizeof(float)); step_down(a->s0b, s0b.p, s0b.n * sizeof(float)); }
        if (a->s1T) { step_down(a->s1T, s1T.p, s1T.n * sizeof(float)); step_down(a->s1b, s1b.p, s1b.n * sizeof(float)); }
        for (int i = 0; i < 2; ++i)
            if (a->plane_kind[i]) { step_down(a->planes[i], planes[i].p, planes[i].n); step_down(a->fresh[i], fresh[i].p, fresh[i].n); }
    });
}

}  // extern "C"
