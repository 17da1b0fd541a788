// Stand-alone host program for tests/test_treeset_plan_cpu.py: prints the plan of every scored-tree-set call (chunk, grid, bytes
// per tree, node store of a workgroup, total and every offset) over a thinned grid of shapes, one line per plan, in the format of
// tests/golden/treeset_plans.txt, which holds the same lines as the plan functions gave them before they shared one slab builder.
// A line is "call inputs... : outputs..."; a loglik line carries "| total offsets..." behind the outputs that must not move.
#include <stdio.h>

#include <vector>

#include "phylo_treeanc_rates.h"
#include "phylo_treegrad_model.h"
#include "phylo_treenni_rates.h"
#include "phylo_treeset.h"

static const int Ns[] = {2, 3, 4, 5, 12, 33, 70, 128, 511, 512};
static const int NTs[] = {1, 2, 3, 64};
static const int Ts[] = {1, 5, 37, 4096, 1 << 20};
static const int CUs[] = {1, 64, 256, 304};
static const int ENVs[] = {0, 1, 5};
static const int Cs[] = {1, 4, 16};
static const int Ps[] = {1, 16};
static const int Ss[] = {1, 130, 50000};

struct shape {
    int N, nt, T, cu, env, coded, C, P, S, opt;   // opt: a counter the call takes its option bits from
};

// Two thinned sub-grids: every N three times with T stepping through its values, and every (ntiles, n_cus) pair; the other inputs
// cycle with the index at strides of their own, so that every value of every input meets several values of the others.  Half the
// shapes have no chunk cap (env_chunk 0): those are the plans whose chunk comes from the budget.
static std::vector<shape> shapes() {
    static const int envs[] = {0, 1, 0, 5};
    std::vector<shape> v;
    for (int i = 0; i < 30; ++i)
        v.push_back({Ns[i % 10], NTs[i % 4], Ts[(i + i / 10) % 5], CUs[(i / 2) % 4], envs[(i / 3) % 4], i % 2, Cs[(i / 2) % 3], Ps[(i / 5) % 2],
                     Ss[(i / 4) % 3], i});
    int i = 30;
    for (int nt : NTs)
        for (int cu : CUs) {
            v.push_back({Ns[(3 * i) % 10], nt, Ts[(2 * i + i / 5) % 5], cu, envs[i % 4], (i / 2) % 2, Cs[i % 3], Ps[i % 2], Ss[(i / 2) % 3], i});
            ++i;
        }
    return v;
}

#define Z(x) printf(" %zu", (size_t)(x))

// one plain and one rates line; the depths of the T trees of the rates call: all deep, all shallow, or shallow in the last tree alone
static void loglik_rows(const shape& s) {
    for (int mix = 0; mix < 2; ++mix) {
        const int want_sites = mix ? (s.opt / 3) % 2 : s.opt % 2, pattern = mix ? s.opt % 3 : 0, want_cat = mix && (s.opt & 1);
        const int nc = mix ? s.C : 1;
        std::vector<int> depth_of(mix ? (size_t)s.T : 0);
        for (int t = 0; t < (int)depth_of.size(); ++t) depth_of[t] = pattern == 0 ? 7 : pattern == 1 ? 2 : (t == s.T - 1 ? 1 : 5);
        pt2_plan p;
        const int rc = pt2_make_plan(s.N, s.S, s.nt, s.T, nc, mix != 0, s.coded != 0, want_sites != 0, want_cat != 0, s.env,
                                     mix ? depth_of.data() : nullptr, &p);
        printf("pt2 %d %d %d %d %d %d %d %d %d %d %d : %d %d %d", s.N, s.S, s.nt, s.T, nc, mix, s.coded, want_sites, want_cat, s.env, pattern, rc,
               p.chunk, (int)p.sites);
        Z(p.per_tree);
        printf(" |");
        Z(p.total); Z(p.o_prior); Z(p.o_ops); Z(p.o_P); Z(p.o_t); Z(p.o_gap); Z(p.o_tilev); Z(p.o_out); Z(p.o_site); Z(p.o_cat);
        printf("\n");
    }
}

int main() {
    for (const shape& s : shapes()) {
        const bool coded = s.coded != 0;
        loglik_rows(s);
        {
            const int curv = (s.opt / 2) & 1;
            ptg_plan p;
            const int rc = ptg_make_plan(s.N, s.nt, s.T, coded, curv != 0, s.cu, s.env, &p);
            printf("ptg %d %d %d %d %d %d %d : %d %d %d %d", s.N, s.nt, s.T, s.coded, curv, s.cu, s.env, rc, p.chunk, p.grid, p.nq);
            Z(p.per_tree); Z(p.wg_store); Z(p.total); Z(p.o_prior); Z(p.o_ops); Z(p.o_dops); Z(p.o_P); Z(p.o_t); Z(p.o_gap); Z(p.o_tilev); Z(p.o_out);
            Z(p.o_dtile); Z(p.o_dout); Z(p.o_store);
            printf("\n");
        }
        {
            const int curv = s.opt & 1, params = (s.opt >> 1) & 1;
            ptgr_plan p;
            const int rc = ptgr_make_plan(s.N, s.nt, s.T, s.C, coded, curv != 0, params != 0, s.cu, s.env, &p);
            printf("ptgr %d %d %d %d %d %d %d %d %d : %d %d %d %d %d %d", s.N, s.nt, s.T, s.C, s.coded, curv, params, s.cu, s.env, rc, p.chunk, p.grid,
                   p.nq, p.np, p.ncoef);
            Z(p.per_tree); Z(p.wg_store); Z(p.total); Z(p.o_prior); Z(p.o_coef); Z(p.o_ops); Z(p.o_dops); Z(p.o_P); Z(p.o_t); Z(p.o_b); Z(p.o_gap);
            Z(p.o_tilev); Z(p.o_out); Z(p.o_dtile); Z(p.o_dout); Z(p.o_ptile); Z(p.o_pout); Z(p.o_store);
            printf("\n");
        }
        {
            const int grad = (s.opt / 3) & 1;
            ptm_plan p;
            const int rc = ptm_make_plan(s.N, s.nt, s.T, s.P, coded, grad != 0, s.cu, s.env, &p);
            printf("ptm %d %d %d %d %d %d %d %d : %d %d %d %d", s.N, s.nt, s.T, s.P, s.coded, grad, s.cu, s.env, rc, p.chunk, p.grid, p.nm);
            Z(p.per_tree); Z(p.wg_store); Z(p.total); Z(p.o_prior); Z(p.o_dirs); Z(p.o_ops); Z(p.o_dops); Z(p.o_P); Z(p.o_D); Z(p.o_t); Z(p.o_gap);
            Z(p.o_tilev); Z(p.o_out); Z(p.o_dtile); Z(p.o_dout); Z(p.o_mtile); Z(p.o_mout); Z(p.o_store);
            printf("\n");
        }
        {
            ptn_plan p;
            const int rc = ptn_make_plan(s.N, s.nt, s.T, coded, s.cu, s.env, &p);
            printf("ptn %d %d %d %d %d %d : %d %d %d", s.N, s.nt, s.T, s.coded, s.cu, s.env, rc, p.chunk, p.grid);
            Z(p.per_tree); Z(p.wg_store); Z(p.total); Z(p.o_prior); Z(p.o_ops); Z(p.o_dops); Z(p.o_nops); Z(p.o_P); Z(p.o_t); Z(p.o_gap); Z(p.o_tilev);
            Z(p.o_out); Z(p.o_dtile); Z(p.o_dout); Z(p.o_store);
            printf("\n");
        }
        {
            ptnr_plan p;
            const int rc = ptnr_make_plan(s.N, s.nt, s.T, s.C, coded, s.cu, s.env, &p);
            printf("ptnr %d %d %d %d %d %d %d : %d %d %d", s.N, s.nt, s.T, s.C, s.coded, s.cu, s.env, rc, p.chunk, p.grid);
            Z(p.per_tree); Z(p.wg_store); Z(p.total); Z(p.o_prior); Z(p.o_w); Z(p.o_ops); Z(p.o_dops); Z(p.o_nops); Z(p.o_P); Z(p.o_t); Z(p.o_gap);
            Z(p.o_tilev); Z(p.o_out); Z(p.o_dtile); Z(p.o_dout); Z(p.o_store);
            printf("\n");
        }
        {
            const unsigned outs = 1u + (unsigned)(s.opt % 7);
            pta_plan p;
            const int rc = pta_make_plan(s.N, s.S, s.nt, s.T, coded, outs, s.cu, s.env, &p);
            printf("pta %d %d %d %d %d %u %d %d : %d %d %d", s.N, s.S, s.nt, s.T, s.coded, outs, s.cu, s.env, rc, p.chunk, p.grid);
            Z(p.per_tree); Z(p.wg_store); Z(p.out_tree); Z(p.out_region); Z(p.total); Z(p.o_prior); Z(p.o_ops); Z(p.o_dops); Z(p.o_P); Z(p.o_t);
            Z(p.o_gap); Z(p.o_tilev); Z(p.o_out); Z(p.o_post); Z(p.o_state); Z(p.o_pmax); Z(p.o_store);
            printf("\n");
        }
        {
            const unsigned outs = 1u + (unsigned)((s.opt * 5) % 31);
            ptar_plan p;
            const int rc = ptar_make_plan(s.N, s.S, s.nt, s.T, s.C, coded, outs, s.cu, s.env, &p);
            printf("ptar %d %d %d %d %d %d %u %d %d : %d %d %d %d", s.N, s.S, s.nt, s.T, s.C, s.coded, outs, s.cu, s.env, rc, p.chunk, p.grid, p.ncoef);
            Z(p.per_tree); Z(p.wg_store); Z(p.out_tree); Z(p.out_region); Z(p.total); Z(p.o_prior); Z(p.o_coef); Z(p.o_ops); Z(p.o_dops); Z(p.o_P);
            Z(p.o_t); Z(p.o_gap); Z(p.o_tilev); Z(p.o_out); Z(p.o_post); Z(p.o_state); Z(p.o_pmax); Z(p.o_cat); Z(p.o_rate); Z(p.o_store);
            printf("\n");
        }
    }
    return 0;
}
