// options.hip — the table behind options.h: names, environment variables, defaults and permitted values of the runtime switches.
#include "options.h"
#include "../../include/dm_engine.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace dm {

namespace {
struct OptDef { const char* name; const char* env; int def; };
const OptDef kOpts[OPT_COUNT] = {
    {"igemm_big", "DM_IGEMM_BIG", -1}, {"igemm_splitk", "DM_IGEMM_SPLITK", 1},
    {"ln_fold", "DM_LN_FOLD", 1}, {"attn_pipe", "DM_ATTN_PIPE", 1}, {"igemm_tail", "DM_IGEMM_TAIL", 1}, {"attn_cross", "DM_ATTN_CROSS", 1}, {"ln_stats_g", "DM_LN_STATS_G", 1}, {"igemm_exp", "DM_IGEMM_EXP", 0}, {"ln_inkernel", "DM_LN_INKERNEL", 1}, {"graph", "DM_GRAPH", 0}, {"gn_fold", "DM_GN_FOLD", 1}, {"sc_fold", "DM_SC_FOLD", 1}, {"ff_fold", "DM_FF_FOLD", 1}, {"tap_reuse", "DM_TAP_REUSE", 1}, {"up_fold", "DM_UP_FOLD", 1}, {"q_once", "DM_Q_ONCE", 1}, {"gn_epi", "DM_GN_EPI", 1}, {"conv_out_rows", "DM_CONV_OUT_ROWS", 1}, {"gn_skip", "DM_GN_SKIP", 1},
};
// The values a switch may take: attn_pipe selects kernels by number, and a number outside the list used to fall through to
// whatever instantiation the launcher's switch held (timing-only ablations included).  Every other switch is 0 / 1 / 2 / -1 by meaning.
static bool option_value_ok(int i, int value) {
    if (i == OPT_ATTN_PIPE) {
#ifdef DM_ATTN_PP_ABLATE
        return value >= 0 && value <= 51;
#else
        return value == 0 || value == 1 || value == 2 || value == 3 || value == 5 || value == 6 || value == 9 || value == 10 || value == 12;
#endif
    }
    if (i == OPT_IGEMM_BIG) return value >= -1 && value <= 2;
    return value >= 0 && value <= 2;
}
std::atomic<int> g_opt[OPT_COUNT];
std::atomic<int> g_opt_init{0};
std::atomic<unsigned> g_opt_epoch{1};      // bumped by every set_option(): engines drop cached arena peaks and captured graphs
void opts_init() {
    if (g_opt_init.load() == 2) return;
    int expect = 0;
    if (g_opt_init.compare_exchange_strong(expect, 1)) {
        for (int i = 0; i < OPT_COUNT; ++i) {
            const char* e = getenv(kOpts[i].env);
            int v = e ? atoi(e) : kOpts[i].def;
            if (e && !option_value_ok(i, v)) {              // an environment value outside the switch's set: say so and keep the default
                fprintf(stderr, "dm_engine: %s=%s is not a value of option \"%s\"; using the default %d\n", kOpts[i].env, e, kOpts[i].name, kOpts[i].def);
                v = kOpts[i].def;
            }
            g_opt[i] = v;
        }
        g_opt_init = 2;
    } else while (g_opt_init.load() != 2) {}
}
}  // namespace

int option(Option o) { opts_init(); return g_opt[o].load(std::memory_order_relaxed); }
unsigned options_epoch() { return g_opt_epoch.load(std::memory_order_relaxed); }
int get_option(const char* name, int* value) {
    opts_init();
    for (int i = 0; i < OPT_COUNT; ++i)
        if (name && value && !strcmp(name, kOpts[i].name)) { *value = g_opt[i].load(); return 0; }
    return 1;
}
int set_option(const char* name, int value) {
    opts_init();
    for (int i = 0; i < OPT_COUNT; ++i)
        if (name && !strcmp(name, kOpts[i].name)) {
            if (!option_value_ok(i, value)) return 2;          // known switch, value outside its documented set: refused, nothing changes
            if (g_opt[i].exchange(value) != value) g_opt_epoch.fetch_add(1);
            return 0;
        }
    return 1;
}

}  // namespace dm

extern "C" {

int dm_set_option(const char* name, int value) { return dm::set_option(name, value); }
int dm_get_option(const char* name, int* value) { return dm::get_option(name, value); }

}  // extern "C"
