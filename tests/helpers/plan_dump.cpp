// Prints the whole host-side plan (csrc/net_plan.h) of every configuration on stdin: tests/test_plan_snapshot_host.py compares the
// text with tests/golden/plan_snapshot.txt, which oracle/make_golden_plan.py recorded.  Host only: nothing here touches a device.
//
//   plan_dump [--all] < configurations
//
// One configuration per line, the fields of isdqn_net_config in declaration order (tests/helpers/plan_grid.py writes them): integers
// in decimal, floats as C hex floats; the line "null" stands for a null pointer.  Per line: "== <line>", "rc <code>", then the
// last-error text of a refusal without its " (file:line)", or every plan field the configuration defines, one line per struct.
// --all prints every field of every array element instead, used or not.
#include <stdarg.h>

#include "net_plan.h"

namespace isdqn {
static char last_error[512];
void set_last_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error, sizeof(last_error), fmt, ap);
    va_end(ap);
}
}  // namespace isdqn

using namespace isdqn;

#define I(s, f) printf(" " #f "=%lld", (long long)(s).f)

static void dump_layer(const char* pre, const Layer& l, bool all) {
    printf("%s", pre);
    I(l, kind); I(l, has_ln); I(l, has_relu); I(l, is_head);
    I(l, hin); I(l, win); I(l, cin); I(l, cin_p); I(l, hout); I(l, wout); I(l, cout); I(l, cout_p); I(l, ksz); I(l, stride); I(l, pad);
    I(l, taps); I(l, npix); I(l, is_u8);
    I(l, in_f); I(l, in_p); I(l, in_unpadded_ld); I(l, out_f); I(l, out_p); I(l, K); I(l, in_elems_p); I(l, out_elems_p);
    I(l, w_off); I(l, b_off); I(l, g_off); I(l, be_off); I(l, w_size);
    I(l, act_off); I(l, z_off); I(l, dz_off); I(l, gw_off); I(l, part_off);
    I(l, gw_slabs); I(l, fwd_splits); I(l, fwd_narrow);
    if (all || l.wgi_ntw > 0) { I(l, wgi_ntw); I(l, wgi_G); I(l, wgi_groups); }
    I(l, dgi_tiles);
    if (all || l.dgi_tiles > 0) I(l, dgi_tile_pix);
    I(l, red_off); I(l, part_rows);
    printf(" name=%.*s ln_name=%.*s\n", (int)sizeof(l.name), l.name, (int)sizeof(l.ln_name), l.ln_name);
}

static void dump_stack(int s, const ImpalaStack& S, bool all) {
    printf("imp[%d]", s);
    I(S, H); I(S, W); I(S, Hp); I(S, Wp); I(S, pool_pad); I(S, cin); I(S, cin_p); I(S, C); I(S, C_p);
    for (int b = 0; b < 2; ++b) printf(" ln_g[%d]=%lld ln_b[%d]=%lld", b, (long long)S.ln_g[b], b, (long long)S.ln_b[b]);
    I(S, xin_off); I(S, z0_off); I(S, arg_off);
    for (int k = 0; k < 3; ++k) printf(" r_off[%d]=%lld", k, (long long)S.r_off[k]);
    for (int b = 0; b < 2; ++b)
        printf(" a1_off[%d]=%lld a2_off[%d]=%lld lnpart_off[%d]=%lld", b, (long long)S.a1_off[b], b, (long long)S.a2_off[b], b,
               (long long)S.lnpart_off[b]);
    I(S, zt_off); I(S, dr_off); I(S, da_off); I(S, dzs_off); I(S, dz0_off);
    for (int k = 0; k < IMP_CONVS; ++k) printf(" bpart_off[%d]=%lld", k, (long long)S.bpart_off[k]);
    printf("\n");
    for (int k = 0; k < IMP_CONVS; ++k) {
        char pre[32];
        snprintf(pre, sizeof(pre), "imp[%d].conv[%d]", s, k);
        dump_layer(pre, S.conv[k], all);
    }
}

static void dump_bn(int s, const BnSite& b) {
    printf("bns[%d]", s);
    I(b, layer); I(b, spatial); I(b, P); I(b, C); I(b, Cp); I(b, G); I(b, G_p);
    I(b, scale_off); I(b, bias_off); I(b, mean_off); I(b, var_off);
    I(b, in_off); I(b, out_off); I(b, bmean_off); I(b, bvar_off); I(b, s1_off); I(b, s2_off);
    printf(" name=%.*s\n", (int)sizeof(b.name), b.name);
}

// one line per struct -- "P", "L[i]", "imp[s]", "imp[s].conv[k]", "bns[s]" -- of " field=value" tokens, then the regions in order
static void dump_plan(const isdqn_net_config& cfg, const Plan& P, bool all) {
    printf("P");
    I(P, n_layers); I(P, B); I(P, N2); I(P, bn); I(P, Bb); I(P, n_bn); I(P, x0_off);
    I(P, n_heads); I(P, n_actions); I(P, nha); I(P, nha_p); I(P, nlog); I(P, nlog_p); I(P, head_nb); I(P, qr); I(P, c51);
    printf(" hl_min=%a hl_max=%a hl_sigma=%a", P.hl_min, P.hl_max, P.hl_sigma);
    I(P, K); I(P, oh); I(P, n_params);
    I(P, q_off); I(P, logits_off); I(P, out_off); I(P, dout_off); I(P, da_off); I(P, slab_off); I(P, qv_off); I(P, tg_off); I(P, dbh_off);
    I(P, adam_tab_off); I(P, lpart_off);
    I(P, double_q); I(P, qt_rows); I(P, munchausen); I(P, qt_off); I(P, logits_t_off); I(P, out_t_off);
    I(P, dueling); I(P, raw); I(P, raw_p); I(P, duel_f); I(P, duel_f2); I(P, raw_off); I(P, raw_t_off); I(P, dout_raw_off); I(P, dbh_raw_off);
    I(P, grad_clip); I(P, gc_part_off); I(P, gc_off); I(P, gc_part_cap);
    I(P, wsplit_off); I(P, slab_floats); I(P, da_floats); I(P, ws_bytes);
    printf("\n");
    const int nl = all ? MAX_LAYERS : P.n_layers;
    for (int i = 0; i < nl; ++i) {
        char pre[16];
        snprintf(pre, sizeof(pre), "L[%d]", i);
        dump_layer(pre, P.L[i], all);
    }
    if (all || cfg.arch == ISDQN_ARCH_IMPALA)
        for (int s = 0; s < IMP_STACKS; ++s) dump_stack(s, P.imp[s], all);
    const int nb = all ? (int)(sizeof(P.bns) / sizeof(P.bns[0])) : P.n_bn;
    for (int s = 0; s < nb; ++s) dump_bn(s, P.bns[s]);
    printf("regions");
    for (auto& r : P.regions) printf(" %s=%lld+%lld", r.first.c_str(), (long long)r.second.first, (long long)r.second.second);
    printf("\n");
}

static bool parse(char* line, isdqn_net_config& c) {
    int32_t* ints[] = {&c.arch, &c.obs_h, &c.obs_w, &c.obs_c, &c.n_features, &c.features[0], &c.features[1], &c.features[2], &c.features[3],
                       &c.features[4], &c.features[5], &c.features[6], &c.features[7], &c.n_actions, &c.n_heads, &c.dueling, &c.layer_norm,
                       &c.batch_size, &c.precision};
    float* floats[] = {&c.gamma_n, &c.learning_rate, &c.adam_b1, &c.adam_b2, &c.adam_eps, &c.max_grad_norm, &c.huber_delta, &c.munchausen_tau,
                       &c.munchausen_alpha, &c.munchausen_clip};
    int32_t* ints2[] = {&c.batch_norm, &c.categorical, &c.n_bins, &c.n_quantiles};
    float* floats2[] = {&c.hl_min, &c.hl_max, &c.hl_sigma};
    static_assert(ISDQN_MAX_FEATURES == 8 && sizeof(isdqn_net_config) == 4 * (19 + 10 + 4 + 3 + 1), "a field this parser does not read");
    char* p = line;
    char* end;
    for (int32_t* f : ints) { *f = (int32_t)strtol(p, &end, 10); if (end == p) return false; p = end; }
    for (float* f : floats) { *f = strtof(p, &end); if (end == p) return false; p = end; }
    for (int32_t* f : ints2) { *f = (int32_t)strtol(p, &end, 10); if (end == p) return false; p = end; }
    for (float* f : floats2) { *f = strtof(p, &end); if (end == p) return false; p = end; }
    c.double_q = (int32_t)strtol(p, &end, 10);
    if (end == p) return false;
    while (*end == ' ') ++end;
    return *end == 0;
}

int main(int argc, char** argv) {
    const bool all = argc > 1 && strcmp(argv[1], "--all") == 0;
    char line[1024];
    while (fgets(line, sizeof(line), stdin)) {
        line[strcspn(line, "\r\n")] = 0;
        if (!line[0]) continue;
        printf("== %s\n", line);
        isdqn_net_config cfg;
        memset(&cfg, 0, sizeof(cfg));
        const bool null = strcmp(line, "null") == 0;
        if (!null && !parse(line, cfg)) {
            fprintf(stderr, "plan_dump: cannot parse '%s'\n", line);
            return 2;
        }
        Plan P;  // default-initialised on purpose: the test builds this file with -ftrivial-auto-var-init=zero and =pattern
        last_error[0] = 0;
        const int rc = build_plan(null ? nullptr : &cfg, P);
        printf("rc %d\n", rc);
        if (rc) {
            if (char* tail = strrchr(last_error, '(')) {
                if (tail > last_error && tail[-1] == ' ') tail[-1] = 0;
            }
            printf("%s\n", last_error);
        } else {
            dump_plan(cfg, P, all);
        }
    }
    return 0;
}
