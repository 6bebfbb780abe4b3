// Integer tuning options of a handle, driven from ONE table per handle type: a row names the option, its environment variable, the member it sets and what it
// accepts.  cv_*_set_option looks a name up and stores through option_store(); cv_*_finalize applies the environment through the same function, so a value is
// checked the same way wherever it comes from.
#pragma once
#include <climits>
#include <cstdlib>
#include <cstring>
#include "api_common.h"

namespace cv {

// Options that select a measured no-go (kept as evidence, built only with -DCV_BUILD_EXPERIMENTS: VERDICT r5 item 9)
#ifdef CV_BUILD_EXPERIMENTS
static constexpr bool kExperiments = true;
#else
static constexpr bool kExperiments = false;
#endif
static inline void need_experiments(bool wanted, const std::string& what) {
    if (wanted && !kExperiments) throw Error(what + " selects an experiment this library was built without (rebuild with CV_BUILD_EXPERIMENTS=1)");
}

constexpr int kAnyBuild = INT_MIN;      // Option::product: not gated
template <typename H>
struct Option {
    const char* name;
    const char* env;            // environment variable applied at finalize, or null
    int H::*field;
    bool boolean;               // store value != 0
    int lo, hi;                 // legal closed range ...
    int n_values, values[4];    // ... or, when n_values > 0, the legal values
    int product;                // the only (stored) value a library built without CV_BUILD_EXPERIMENTS accepts; kAnyBuild = every legal value
    bool drops_graphs;          // captured graphs bake the choice in: the caller drops them after a store
};

template <typename H>
static std::string option_legal(const Option<H>& o) {
    std::string s;
    for (int i = 0; i < o.n_values; ++i) s += (i == 0 ? "" : i + 1 == o.n_values ? " or " : ", ") + std::to_string(o.values[i]);
    return o.n_values > 0 ? s : o.hi == INT_MAX ? ">= " + std::to_string(o.lo) : std::to_string(o.lo) + " .. " + std::to_string(o.hi);
}

// Checks `value` against the row and stores it.  `who` leads the messages ("flow option", "llm option", or "<VARIABLE>: flow option").
template <typename H>
static void option_store(H* h, const Option<H>& o, int value, const std::string& who) {
    bool ok = o.boolean || (value >= o.lo && value <= o.hi);
    if (!o.boolean && o.n_values > 0) { ok = false; for (int i = 0; i < o.n_values; ++i) ok = ok || value == o.values[i]; }
    if (!ok) throw Error(who + " " + o.name + " must be " + option_legal(o) + " (got " + std::to_string(value) + ")");
    if (o.boolean) value = value != 0;
    need_experiments(o.product != kAnyBuild && value != o.product, who + " " + o.name + " = " + std::to_string(value));
    h->*o.field = value;
}

// cv_*_set_option: the row called `name` after the store, null when the table has no such option (the caller's special cases, then "unknown option")
template <typename H, size_t N>
static const Option<H>* option_set(H* h, const Option<H> (&table)[N], const char* name, int value, const char* who) {
    for (const auto& o : table)
        if (std::strcmp(o.name, name) == 0) { option_store(h, o, value, who); return &o; }
    return nullptr;
}

// cv_*_finalize: every variable that is set, as a whole decimal integer, through option_store
template <typename H, size_t N>
static void option_apply_env(H* h, const Option<H> (&table)[N], const char* who) {
    for (const auto& o : table) {
        const char* e = o.env ? getenv(o.env) : nullptr;
        if (!e) continue;
        char* end = nullptr;
        const long v = strtol(e, &end, 10);
        if (end == e || *end != '\0' || v < INT_MIN || v > INT_MAX) throw Error(std::string(o.env) + "='" + e + "' is not an integer (" + who + " " + o.name + ")");
        option_store(h, o, (int)v, std::string(o.env) + ": " + who);
    }
}

}  // namespace cv
