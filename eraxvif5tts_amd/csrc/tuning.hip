// tuning.hip -- the tuning knobs' definitions (defaults from the table of tuning.h) and the entry points that set, read and list them.  No kernel.
#include "tuning.h"

#include <string.h>

#include "common.h"

#define F5_KNOB_DEFINE(key, var, def, kind, check) int var = def;
F5_TUNING_KNOBS(F5_KNOB_DEFINE)
#undef F5_KNOB_DEFINE

int g_tuning_epoch = 0;

namespace {
enum Kind { INT, BOOL };

// validators of the table: null = accepted, otherwise why the value is refused
const char* ANY(int) { return nullptr; }
const char* bigvgan_group_frames_positive(int v) { return v < 1 ? "bigvgan_group_frames must be at least 1" : nullptr; }
const char* gemm_persist_grid_in_range(int v) { return v != 0 && (v < 8 || v > 4096) ? "gemm_persist_grid must be 0 (= CU count) or in [8, 4096]" : nullptr; }
const char* attn_variant_known(int v) {
    return v == 6 ? "attn_variant 6 (the persistent-grid kernel) was removed: 0 = by grid size, 2 = 64 queries per wave, 5 = pipelined" : nullptr;
}

struct Knob {
    const char* key;
    int* var;
    Kind kind;
    const char* (*refuse)(int);
};
#define F5_KNOB_ROW(key, var, def, kind, check) {key, &var, kind, check},
const Knob KNOBS[] = {F5_TUNING_KNOBS(F5_KNOB_ROW)};
#undef F5_KNOB_ROW
const int N_KNOBS = (int)(sizeof(KNOBS) / sizeof(KNOBS[0]));

const Knob* find_knob(const char* key) {
    for (const Knob& k : KNOBS)
        if (strcmp(key, k.key) == 0) return &k;
    return nullptr;
}
}  // namespace

extern "C" int f5_tuning_set(const char* key, int value) {
    if (!key) return f5_fail(F5_EINVAL, "null key");
    ++g_tuning_epoch;  // hipGraphs captured by plans under the previous knob values are dropped at their next use (model.hip)
    const Knob* k = find_knob(key);
    if (!k) return f5_fail(F5_EINVAL, "unknown tuning key '%s'", key);
    if (const char* why = k->refuse(value)) return f5_fail(F5_EINVAL, "%s", why);
    *k->var = k->kind == BOOL ? value != 0 : value;
    return 0;
}

extern "C" int f5_tuning_get(const char* key, int* value) {
    if (!key || !value) return f5_fail(F5_EINVAL, "null argument");
    const Knob* k = find_knob(key);
    if (!k) return f5_fail(F5_EINVAL, "unknown tuning key '%s'", key);
    *value = *k->var;
    return 0;
}

extern "C" const char* f5_tuning_key(int index) { return index >= 0 && index < N_KNOBS ? KNOBS[index].key : nullptr; }
