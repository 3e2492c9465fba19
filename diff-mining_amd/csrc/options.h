// options.h — the process-wide runtime switches.  Stands alone (f32_impl.h), and is what dm_kernels.h includes from inside its own
// `namespace dm` (DM_OPTIONS_IN_NAMESPACE_DM), so the kernels' translation units see these declarations where they always stood.
#pragma once
#ifndef DM_OPTIONS_IN_NAMESPACE_DM
namespace dm {
#endif

// Runtime switches (A/B measurements; every default is the measured best).  Initialised from the environment variable of
// the same name in upper case with a DM_ prefix (DM_IGEMM_PERSIST=0 ...), changeable through dm_set_option().
enum Option { OPT_IGEMM_BIG = 0, OPT_IGEMM_SPLITK, OPT_LN_FOLD, OPT_ATTN_PIPE, OPT_IGEMM_TAIL, OPT_ATTN_CROSS, OPT_LN_STATS_G, OPT_IGEMM_EXP, OPT_LN_INKERNEL, OPT_GRAPH, OPT_GN_FOLD, OPT_SC_FOLD, OPT_FF_FOLD, OPT_TAP_REUSE, OPT_UP_FOLD, OPT_Q_ONCE, OPT_GN_EPI, OPT_CONV_OUT_ROWS, OPT_GN_SKIP, OPT_COUNT };
int option(Option o);                       // options.hip
unsigned options_epoch();                   // options.hip: changes with every set_option() that changed a value
int set_option(const char* name, int value);   // 0 on success
int get_option(const char* name, int* value);  // 0 on success

#ifndef DM_OPTIONS_IN_NAMESPACE_DM
}  // namespace dm
#endif
