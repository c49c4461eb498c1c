// The wave engine's headline kernels compiled at run time for the constants of one context.
// Host only: sf_api.hip includes it after sf_wave_plan.h.  The COMPACT FAST + SMALL kernel of launch modes 3 / 4 / 5 is bound by instruction
// issue with both register files full, and most of what its scalar registers and spill lanes hold never changes for the life of a context:
// V, dim, n_cap, the two max_nearby and everything derived from them.  wave_spec_wanted -- a pure function beside plan_wave_launch -- says
// whether a launch should run a kernel compiled for those constants; wave_spec_get compiles csrc/sf_tu_list_wave_spec.hip in process through
// hiprtc (loaded with dlopen: no link dependency, the library loads where hiprtc is absent) and keeps the module in a process-wide cache.
// Any failure is remembered for its key and the launch goes through the ahead-of-time kernel.  The structs hold int32 fields only:
// sf_debug_wave_spec / sf_debug_wave_spec_gate hand them to the tests as flat arrays in declaration order.
// The key also carries three facts of the context's neighbour index (sf_nbr_facts.h) and the candidates that rest on them:
// wave_spec_index_allowed -- pure, like wave_spec_wanted -- says which of them a key may compile in.
#pragma once
#include <dlfcn.h>

#include "sf_nbr_facts.h"

#include <fstream>
#include <mutex>
#include <sstream>

// What the specialised kernel is compiled for.
struct WaveSpecKey {
    int32_t levels, wpe;            // the instantiation: score levels 2 / 4, waves per SIMD 4 / 5 / 6 (launch mode 3 / 4 / 5)
    int32_t V, dim, n_cap, k0, k1;  // ListModel::V / dim / n_cap, max_nearby of leaf 0 and of leaf 1
    // the candidates beyond those five: `extras` = the SF_WSPEC_X_* bits compiled in; the fields of a bit that is off are zero
    int32_t extras;
    int32_t capacity, cap_weight, dist_weight, depot, cap_level, dist_level;  // SF_WSPEC_X_MODEL: level_words' inputs
    int32_t la_size, limit, has_perm, has_explicit;                           // SF_WSPEC_X_LA / _LIMIT / _PERM / _EXPLICIT
    // Facts of the context's neighbour index as three flags, and `index_x` = the SF_WSPEC_X_* bits compiled in that rest on them.
    // These words come after the eighteen above, which keep their places and meanings: a caller that hands over eighteen words names a key
    // of unknown facts and no such candidate.
    int32_t wide_ties, ties, rows_full;  // some equal-distance group has 64 members or more; some group has two; every row has min(dim, 64) finite entries
    int32_t index_x;
    // A fact of the matrix the kernel gathers its legs from (sf_mat_facts.h), behind the twenty-two words above: a caller that hands
    // over twenty-two names a matrix nobody has looked at.  The two leg candidates live in `index_x` with the index's.
    int32_t mat_sym;  // mat[a][b] == mat[b][a] for every pair of the compact matrix, the not-finite word included
};
constexpr int32_t SF_WSPEC_KEY_WORDS_V2 = 22;  // the key before the matrix's fact: likewise
constexpr int32_t SF_WSPEC_KEY_WORDS_V1 = 18;  // the key before the index's facts: still taken and handed out by the sf_debug_wave_spec* entry points
enum { SF_WSPEC_X_MODEL = 1, SF_WSPEC_X_LA = 2, SF_WSPEC_X_LIMIT = 4, SF_WSPEC_X_PERM = 8, SF_WSPEC_X_EXPLICIT = 16, SF_WSPEC_X_ALL = 31 };
// The candidates that rest on the index's facts: the next bits of SF_AMD_WAVE_SPEC_EXTRAS, kept in the key's `index_x`.
enum { SF_WSPEC_X_NO_WIDE = 32, SF_WSPEC_X_TIE_KEY = 64, SF_WSPEC_X_NO_TIES = 128, SF_WSPEC_X_ROWS_FULL = 256, SF_WSPEC_X_INDEX_ALL = 480 };
// The candidates of the replay batch's leg gathers, the next bits: two legs addressed by their source-side row (rests on the matrix's
// symmetry), and the gathers a lane discards aimed at an address it fetches anyway (rests on nothing).
enum { SF_WSPEC_X_SYM_ROWS = 512, SF_WSPEC_X_LEG_REAIM = 1024, SF_WSPEC_X_LEG_ALL = 1536 };
// The candidates a launch compiles in unless SF_AMD_WAVE_SPEC_EXTRAS says otherwise: those that measured faster than the unit without them,
// alone and on top of each other (profiles/wave_spec_ablation.txt).  The AcceptedCount limit lost 0.4 % alone and gained 0.2 % on
// top of these three; the explicit seeds' absence lost 1.2 % alone and changed nothing on top: both stay arguments.
constexpr int32_t SF_WSPEC_X_DEFAULT = SF_WSPEC_X_MODEL | SF_WSPEC_X_LA | SF_WSPEC_X_PERM;
// Of the index's candidates (profiles/wave_index_facts_ablation.txt), on top of those three: no wide group +1.4 %, the packed tie
// word +2.0 %, full rows +4.7 %, each above the unit without it in every round and each above the pairs it joins; together +7.8 %.  "No
// ties" is never offered for the benchmark's index (it has ties) and so was never measured: it stays a switch.
constexpr int32_t SF_WSPEC_X_INDEX_DEFAULT = SF_WSPEC_X_NO_WIDE | SF_WSPEC_X_TIE_KEY | SF_WSPEC_X_ROWS_FULL;
// Of the leg candidates (profiles/wave_legs_ablation.txt), on top of the six above: the source-side rows +3.9 % alone and +2.2 % on
// top of the re-aimed gathers, above the unit without them in every run; the re-aimed gathers +0.7 % alone and -0.9 % on top of the source-side
// rows, below the unit without them in every run: they stay a switch.
constexpr int32_t SF_WSPEC_X_LEG_DEFAULT = SF_WSPEC_X_SYM_ROWS;
static int32_t wave_spec_extras() {  // diagnostics (the ablation runs): read at every launch
    const char* e = std::getenv("SF_AMD_WAVE_SPEC_EXTRAS");
    return e ? (std::atoi(e) & (SF_WSPEC_X_ALL | SF_WSPEC_X_INDEX_ALL | SF_WSPEC_X_LEG_ALL)) : (SF_WSPEC_X_DEFAULT | SF_WSPEC_X_INDEX_DEFAULT | SF_WSPEC_X_LEG_DEFAULT);
}

// What the candidates' gate reads: the constants the packed word's width follows from, and the facts as the key's flags.
struct WaveSpecIndexGate {
    int32_t V, dim, n_cap;
    int32_t wide_ties, ties, rows_full;
};
static int32_t wave_spec_bits(uint32_t v) {  // bits that hold v (at least one)
    int32_t b = 1;
    while (v >> b) ++b;
    return b;
}
static int32_t wave_spec_rb(int32_t V) { return wave_spec_bits((uint32_t)(V > 1 ? V - 1 : 0)); }
static int32_t wave_spec_pb(int32_t n_cap) { return wave_spec_bits((uint32_t)(n_cap > 0 ? n_cap : 0)); }
// Pure, beside wave_spec_wanted: the index candidates a key of these constants and facts may compile in.  One that its facts do not allow is
// never offered -- the kernel would be wrong, not slow.
static int32_t wave_spec_index_allowed(const WaveSpecIndexGate& g) {
    int32_t a = 0;
    if (!g.wide_ties) a |= SF_WSPEC_X_NO_WIDE;
    if (wave_spec_rb(g.V) + wave_spec_pb(g.n_cap) <= 22) a |= SF_WSPEC_X_TIE_KEY;  // group (6 bits) | ordinal (RB + PB + 1) | weight (2) in one word
    if (!g.ties) a |= SF_WSPEC_X_NO_TIES;
    if (g.rows_full && g.dim >= 32) a |= SF_WSPEC_X_ROWS_FULL;  // (the paired pass reads the first 32 entries of two rows)
    return a;
}
// Pure, beside it: the leg candidates a key of this matrix fact may compile in.  The source-side rows read mat[b][a] where the move's delta is
// defined on mat[a][b]: never offered unless the two are the same word for every pair.
static int32_t wave_spec_leg_allowed(int32_t mat_sym) { return SF_WSPEC_X_LEG_REAIM | (mat_sym ? SF_WSPEC_X_SYM_ROWS : 0); }
// The key of a launch: the instantiation, the model as the kernel sees it, the launch's parameters, the index's facts; `extras` = the
// candidates wanted (one whose value does not fit a literal of its type, or whose facts do not hold, is dropped).
template <class Model, class Params>
static WaveSpecKey wave_spec_key(int32_t levels, int32_t wpe, const Model& m, const Params& q, const NbrFacts& nf, int32_t mat_sym, int32_t extras) {
    WaveSpecKey k{};
    k.levels = levels, k.wpe = wpe, k.V = m.V, k.dim = m.dim, k.n_cap = m.n_cap, k.k0 = q.leaf[0].max_nearby, k.k1 = q.leaf[1].max_nearby;
    k.wide_ties = nf.tie_max >= 64, k.ties = nf.tie_max >= 2, k.rows_full = nf.rows_full != 0;
    k.index_x = extras & SF_WSPEC_X_INDEX_ALL & wave_spec_index_allowed(WaveSpecIndexGate{k.V, k.dim, k.n_cap, k.wide_ties, k.ties, k.rows_full});
    k.mat_sym = mat_sym != 0;
    k.index_x |= extras & SF_WSPEC_X_LEG_ALL & wave_spec_leg_allowed(k.mat_sym);
    extras &= SF_WSPEC_X_ALL;
    auto fits = [](int64_t v) { return v >= INT32_MIN && v <= INT32_MAX; };
    if ((extras & SF_WSPEC_X_MODEL) && !(fits(m.capacity) && fits(m.cap_weight) && fits(m.dist_weight))) extras &= ~SF_WSPEC_X_MODEL;
    if ((m.perm != nullptr) != (m.inv != nullptr)) extras &= ~SF_WSPEC_X_PERM;  // (the two tables come and go together: one switch for both)
    k.extras = extras;
    if (extras & SF_WSPEC_X_MODEL)
        k.capacity = (int32_t)m.capacity, k.cap_weight = (int32_t)m.cap_weight, k.dist_weight = (int32_t)m.dist_weight, k.depot = m.depot, k.cap_level = m.cap_level,
        k.dist_level = m.dist_level;
    if (extras & SF_WSPEC_X_LA) k.la_size = q.la_size;
    if (extras & SF_WSPEC_X_LIMIT) k.limit = q.limit;
    if (extras & SF_WSPEC_X_PERM) k.has_perm = m.perm != nullptr && m.inv != nullptr;
    if (extras & SF_WSPEC_X_EXPLICIT) k.has_explicit = q.explicit_seeds != nullptr;
    return k;
}
// What the policy reads of a launch.
struct WaveSpecGate {
    int32_t mode, move_budget, n_steps;  // the plan's launch mode; the launch has a move budget; its steps (saturated to int32)
    int32_t n_replicas, resident, cus;   // replicas of the launch; resident replicas per CU of the plan; CUs of the device
    int32_t knob;                        // SF_AMD_WAVE_SPEC: 0 never, 1 whenever the mode allows, -1 (unset) the rule
};
enum {  // state of a context's last wave launch, and why
    SF_WSPEC_AOT = 0, SF_WSPEC_SPECIALISED = 1, SF_WSPEC_FELL_BACK = 2,
    SF_WSPEC_R_NONE = 0,
    // ahead-of-time by the policy
    SF_WSPEC_R_KNOB = 1, SF_WSPEC_R_MODE = 2, SF_WSPEC_R_BUDGET = 3, SF_WSPEC_R_STEPS = 4, SF_WSPEC_R_RESIDENCY = 5,
    // fell back
    SF_WSPEC_R_NO_HIPRTC = 10, SF_WSPEC_R_NO_SOURCES = 11, SF_WSPEC_R_COMPILE = 12, SF_WSPEC_R_LOAD = 13, SF_WSPEC_R_LDS = 14,
};
constexpr int32_t SF_WSPEC_MIN_STEPS = 50;  // a compile costs seconds: only launches long enough to be a solve's, never a test's few steps

// Pure: no context, no HIP call, no environment.  Returns SF_WSPEC_R_NONE when the launch should run the specialised kernel, else the reason
// it runs the ahead-of-time one.
static int32_t wave_spec_wanted(const WaveSpecGate& g) {
    if (g.knob == 0) return SF_WSPEC_R_KNOB;
    if (g.mode < 3 || g.mode > 5) return SF_WSPEC_R_MODE;  // the COMPACT FAST + SMALL kernels that keep the node table in LDS
    if (g.knob == 1) return SF_WSPEC_R_NONE;
    if (g.move_budget != 0) return SF_WSPEC_R_BUDGET;  // fixed-step launches only
    if (g.n_steps < SF_WSPEC_MIN_STEPS) return SF_WSPEC_R_STEPS;
    if ((int64_t)g.n_replicas < (int64_t)g.resident * g.cus) return SF_WSPEC_R_RESIDENCY;  // at least one full residency
    return SF_WSPEC_R_NONE;
}
static int32_t wave_spec_knob() {  // read at every launch, like SF_AMD_WAVE_WPB
    const char* e = std::getenv("SF_AMD_WAVE_SPEC");
    return e ? (std::atoi(e) != 0 ? 1 : 0) : -1;
}

// SF_AMD_NO_WAVE_SYM: the unit without the lockstep round (-DSF_WAVE_SYM=0, as a Makefile build takes it through EXTRA).  Read once per process,
// like SF_AMD_NO_COMPACT: the define is not part of the key, so the process-wide cache must never hold both kernels under one key.
static bool wave_spec_no_sym() {
    static const bool once = std::getenv("SF_AMD_NO_WAVE_SYM") != nullptr;
    return once;
}

// The compiler's option list for a key: the Makefile's flags, the target, the include directories, the -D constants.
static std::vector<std::string> wave_spec_options(const WaveSpecKey& k, const std::string& arch, const std::string& csrc, const std::string& rocm_include) {
    auto def = [](const char* name, int32_t v) { return std::string("-D") + name + "(x)=" + std::to_string(v); };
    std::vector<std::string> o{"--offload-arch=" + arch, "-O3", "-std=c++17", "-ffp-contract=off"};
    o.push_back("-I" + csrc);
    if (!rocm_include.empty()) o.push_back("-I" + rocm_include);
    o.push_back("-DSF_SPEC_L=" + std::to_string(k.levels));
    o.push_back("-DSF_SPEC_WPE=" + std::to_string(k.wpe));
    o.push_back(def("SF_SPEC_V", k.V));
    o.push_back(def("SF_SPEC_DIM", k.dim));
    o.push_back(def("SF_SPEC_NCAP", k.n_cap));
    o.push_back(def("SF_SPEC_K0", k.k0));
    o.push_back(def("SF_SPEC_K1", k.k1));
    auto word = [](const char* name, int32_t v) { return std::string("-D") + name + "=(" + std::to_string(v) + ")"; };
    if (k.extras & SF_WSPEC_X_MODEL)
        for (auto& x : {word("SF_SPEC_MODEL_WORDS", 1), word("SF_SPEC_CAPACITY", k.capacity), word("SF_SPEC_CAP_WEIGHT", k.cap_weight), word("SF_SPEC_DIST_WEIGHT", k.dist_weight),
                        word("SF_SPEC_DEPOT", k.depot), word("SF_SPEC_CAP_LEVEL", k.cap_level), word("SF_SPEC_DIST_LEVEL", k.dist_level)})
            o.push_back(x);
    if (k.extras & SF_WSPEC_X_LA) o.push_back(def("SF_SPEC_LA_SIZE", k.la_size));
    if (k.extras & SF_WSPEC_X_LIMIT) o.push_back(def("SF_SPEC_LIMIT", k.limit));
    if (k.extras & SF_WSPEC_X_PERM) o.push_back(def("SF_SPEC_HAS_PERM", k.has_perm));
    if (k.extras & SF_WSPEC_X_EXPLICIT) o.push_back(def("SF_SPEC_HAS_EXPLICIT", k.has_explicit));
    if (k.index_x & SF_WSPEC_X_NO_WIDE) o.push_back(word("SF_SPEC_NO_WIDE", 1));
    if (k.index_x & SF_WSPEC_X_TIE_KEY)
        for (auto& x : {word("SF_SPEC_TIE_KEY", 1), word("SF_SPEC_RB", wave_spec_rb(k.V)), word("SF_SPEC_PB", wave_spec_pb(k.n_cap))}) o.push_back(x);
    if (k.index_x & SF_WSPEC_X_NO_TIES) o.push_back(word("SF_SPEC_NO_TIES", 1));
    if (k.index_x & SF_WSPEC_X_ROWS_FULL) o.push_back(word("SF_SPEC_ROWS_FULL", 1));
    if (k.index_x & SF_WSPEC_X_SYM_ROWS) o.push_back(word("SF_SPEC_SYM_ROWS", 1));
    if (k.index_x & SF_WSPEC_X_LEG_REAIM) o.push_back(word("SF_SPEC_LEG_REAIM", 1));
    if (wave_spec_no_sym()) o.push_back("-DSF_WAVE_SYM=0");
    return o;
}
static std::string wave_spec_kernel_expr(const WaveSpecKey& k) {
    return "sf::k_list_search_wave<" + std::to_string(k.levels) + ", false, 2, true, " + std::to_string(k.wpe) + ", false>";
}
static bool wave_spec_key_ok(const WaveSpecKey& k) {
    return (k.levels == 2 || k.levels == 4) && k.wpe >= 4 && k.wpe <= 6 && k.V >= 1 && k.dim >= 1 && k.n_cap >= 0 && k.k0 >= 1 && k.k1 >= 1 && (k.extras & ~SF_WSPEC_X_ALL) == 0 &&
           (!(k.extras & SF_WSPEC_X_LA) || k.la_size >= 1) && (!(k.extras & SF_WSPEC_X_LIMIT) || k.limit >= 1) &&
           (k.wide_ties | k.ties | k.rows_full | 1) == 1 && (!k.wide_ties || k.ties) &&
           (k.mat_sym | 1) == 1 &&
           (k.index_x & ~(wave_spec_index_allowed(WaveSpecIndexGate{k.V, k.dim, k.n_cap, k.wide_ties, k.ties, k.rows_full}) | wave_spec_leg_allowed(k.mat_sym))) == 0;
}

// hiprtc through dlopen, by its versioned names.
struct WaveSpecRtc {
    void* lib = nullptr;
    std::string include_dir;  // <prefix>/include beside the loaded library's <prefix>/lib
    int (*create)(void**, const char*, const char*, int, const char**, const char**) = nullptr;
    int (*compile)(void*, int, const char**) = nullptr;
    int (*destroy)(void**) = nullptr;
    int (*add_name)(void*, const char*) = nullptr;
    int (*lowered)(void*, const char*, const char**) = nullptr;
    int (*code_size)(void*, size_t*) = nullptr;
    int (*code)(void*, char*) = nullptr;
    int (*log_size)(void*, size_t*) = nullptr;
    int (*log)(void*, char*) = nullptr;
    bool ok() const { return lib && create && compile && destroy && add_name && lowered && code_size && code && log_size && log; }
};
static std::string wave_spec_dirname(const std::string& p) {
    const size_t s = p.find_last_of('/');
    return s == std::string::npos ? std::string(".") : p.substr(0, s);
}
static const WaveSpecRtc& wave_spec_rtc() {
    static const WaveSpecRtc once = [] {
        WaveSpecRtc r;
        for (const char* n : {"libhiprtc.so.7", "libhiprtc.so.6", "libhiprtc.so.5", "libhiprtc.so"})
            if ((r.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
        if (!r.lib) return r;
        auto sym = [&](const char* n) { return dlsym(r.lib, n); };
        r.create = (decltype(r.create))sym("hiprtcCreateProgram");
        r.compile = (decltype(r.compile))sym("hiprtcCompileProgram");
        r.destroy = (decltype(r.destroy))sym("hiprtcDestroyProgram");
        r.add_name = (decltype(r.add_name))sym("hiprtcAddNameExpression");
        r.lowered = (decltype(r.lowered))sym("hiprtcGetLoweredName");
        r.code_size = (decltype(r.code_size))sym("hiprtcGetCodeSize");
        r.code = (decltype(r.code))sym("hiprtcGetCode");
        r.log_size = (decltype(r.log_size))sym("hiprtcGetProgramLogSize");
        r.log = (decltype(r.log))sym("hiprtcGetProgramLog");
        Dl_info di;
        if (r.create && dladdr((void*)r.create, &di) && di.dli_fname) r.include_dir = wave_spec_dirname(wave_spec_dirname(di.dli_fname)) + "/include";
        return r;
    }();
    return once;
}
// The kernel sources: SF_AMD_CSRC, else csrc/ next to the loaded library.
static std::string wave_spec_csrc() {
    if (const char* e = std::getenv("SF_AMD_CSRC")) return e;
    Dl_info di;
    if (dladdr((void*)&wave_spec_csrc, &di) && di.dli_fname) return wave_spec_dirname(di.dli_fname) + "/csrc";
    return "csrc";
}

struct WaveSpecBuild {
    int32_t reason = SF_WSPEC_R_NONE;  // why there is no code (a fall-back reason), or none
    std::vector<char> code;            // the code object
    std::string kernel, log;           // the kernel's lowered name; the compiler's log
    double ms = 0;
};
// One in-process compile.  No device is needed: `arch` names the target.
static WaveSpecBuild wave_spec_compile(const WaveSpecKey& k, const std::string& arch, const std::string& csrc) {
    WaveSpecBuild b;
    const WaveSpecRtc& rtc = wave_spec_rtc();
    if (!rtc.ok()) return b.reason = SF_WSPEC_R_NO_HIPRTC, b;
    static const char* unit = "sf_tu_list_wave_spec.hip";
    std::ifstream f(csrc + "/" + unit, std::ios::binary);
    if (!f) return b.reason = SF_WSPEC_R_NO_SOURCES, b;
    std::stringstream src;
    src << f.rdbuf();
    const std::string text = src.str();
    const auto t0 = std::chrono::steady_clock::now();
    void* prog = nullptr;
    if (rtc.create(&prog, text.c_str(), unit, 0, nullptr, nullptr) != 0 || !prog) return b.reason = SF_WSPEC_R_COMPILE, b;
    const std::string expr = wave_spec_kernel_expr(k);
    const std::vector<std::string> opts = wave_spec_options(k, arch, csrc, rtc.include_dir);
    std::vector<const char*> argv;
    for (auto& o : opts) argv.push_back(o.c_str());
    int rc = rtc.add_name(prog, expr.c_str());
    if (rc == 0) rc = rtc.compile(prog, (int)argv.size(), argv.data());
    size_t n = 0;
    if (rtc.log_size(prog, &n) == 0 && n > 1) {
        b.log.resize(n);
        if (rtc.log(prog, &b.log[0]) != 0) b.log.clear();
    }
    const char* low = nullptr;
    if (rc == 0) rc = rtc.lowered(prog, expr.c_str(), &low);
    if (rc == 0 && low) b.kernel = low;
    if (rc == 0) rc = rtc.code_size(prog, &n);
    if (rc == 0) {
        b.code.resize(n);
        rc = rtc.code(prog, b.code.data());
    }
    (void)rtc.destroy(&prog);
    b.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc != 0 || b.kernel.empty() || b.code.empty()) b.reason = SF_WSPEC_R_COMPILE, b.code.clear();
    return b;
}

// Process-wide cache: one entry per (device, sources, key), failures included.
struct WaveSpecEntry {
    int32_t reason = SF_WSPEC_R_NONE;
    hipModule_t module = nullptr;
    hipFunction_t fn = nullptr;
    int lds_ok = 0;  // dynamic LDS the function's attribute has been raised to
};
struct WaveSpecCache {
    std::mutex mu;
    std::map<std::string, WaveSpecEntry> entries;
    int32_t compiles = 0;  // compiles of the process (attempts that reached the compiler)
    double last_ms = 0;
};
static WaveSpecCache& wave_spec_cache() {
    static WaveSpecCache c;
    return c;
}
// The specialised kernel of `k` on the current device, compiled at the first request.  Returns the entry's reason (none = `fn` is usable for
// a launch with `lds` bytes of dynamic LDS).
static int32_t wave_spec_get(const WaveSpecKey& k, int device, size_t lds, hipFunction_t* fn) {
    WaveSpecCache& c = wave_spec_cache();
    const std::string csrc = wave_spec_csrc();
    std::string id = std::to_string(device) + "|" + csrc;
    const int32_t* w = &k.levels;
    for (size_t i = 0; i < sizeof(WaveSpecKey) / 4; ++i) id += "|" + std::to_string(w[i]);
    std::lock_guard<std::mutex> lock(c.mu);
    auto it = c.entries.find(id);
    if (it == c.entries.end()) {
        WaveSpecEntry e;
        hipDeviceProp_t prop;
        if (!wave_spec_key_ok(k) || hipGetDeviceProperties(&prop, device) != hipSuccess) {
            e.reason = SF_WSPEC_R_COMPILE;
        } else {
            std::string arch = prop.gcnArchName;  // "gfx950:sramecc+:xnack-": the Makefile's target is the processor alone
            arch = arch.substr(0, arch.find(':'));
            WaveSpecBuild b = wave_spec_compile(k, arch, csrc);
            if (b.reason != SF_WSPEC_R_NO_HIPRTC && b.reason != SF_WSPEC_R_NO_SOURCES) c.compiles += 1, c.last_ms = b.ms;
            e.reason = b.reason;
            if (!e.reason && (hipModuleLoadData(&e.module, b.code.data()) != hipSuccess || hipModuleGetFunction(&e.fn, e.module, b.kernel.c_str()) != hipSuccess)) {
                (void)hipGetLastError();
                e.reason = SF_WSPEC_R_LOAD, e.fn = nullptr;
            }
        }
        it = c.entries.emplace(id, e).first;
    }
    WaveSpecEntry& e = it->second;
    if (e.reason) return e.reason;
    // launch_with_lds's twin: the function's dynamic-LDS attribute.  A launch within the 64 KiB every function may take needs none.
    if ((int)lds > e.lds_ok) {
        if (hipFuncSetAttribute((const void*)e.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess) e.lds_ok = (int)lds;
        else {
            (void)hipGetLastError();
            if (lds > 64 * 1024) return SF_WSPEC_R_LDS;  // (this launch only: a smaller one may still run)
        }
    }
    *fn = e.fn;
    return SF_WSPEC_R_NONE;
}
