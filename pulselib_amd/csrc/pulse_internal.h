// pulse_internal.h -- shared by the translation units of libpulse_hip.so (not part of the ABI).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/pulse_env.h"

struct PulseStopRule;
struct ihipStream_t;

namespace pulse {

// Records a thread-local error message and returns `code` (so callers can `return fail(...)`).
int fail(int code, const char* msg);
int fail_hip(int hip_error, const char* what);
// fail(PULSE_EINVAL, "<name>: <msg>"): the argument checks of an entry point that reports under its own name
int fail_named(const char* name, const char* msg);
// After a launch: 0, or fail_hip(hipGetLastError(), what).
int finish_launch(const char* what);
// Compute units of the current device (asked once per device); 256 where the device cannot be asked, with the sticky error cleared.
int device_cus();

// abi.hip: launches `fn` with `lds_bytes` of dynamic LDS.  Beyond the default limit of 48 KiB the limit of `fn` is raised first --
// the first time, and again when a later launch of the same function needs more (the step kernel's size follows obs_size);
// within it no attribute call is made.  `attr`: what raising the limit answered, `launch`: what the launch answered (both
// hipError_t values); after a refusal the launch is tried only with `launch_if_refused`, and then the refusal's sticky error is
// cleared first, so that hipGetLastError() afterwards tells what the LAUNCH answered.
struct LdsLaunch { int attr, launch; };
LdsLaunch launch_lds(const void* fn, unsigned grid, unsigned block, void** params, size_t lds_bytes, ihipStream_t* stream, bool launch_if_refused = false);
// the same for a kernel known by its type: the arguments are checked against its parameters, as a <<< >>> launch checks them
template <class T> struct LdsArg { using type = T; };
template <class... P>
LdsLaunch launch_lds(void (*kernel)(P...), unsigned grid, unsigned block, size_t lds_bytes, ihipStream_t* stream, bool launch_if_refused,
                     typename LdsArg<P>::type... args) {
    void* params[] = {const_cast<void*>(static_cast<const void*>(&args))...};
    return launch_lds(reinterpret_cast<const void*>(kernel), grid, block, params, lds_bytes, stream, launch_if_refused);
}

// abi.hip: workgroups of `block` threads and `lds_bytes` of dynamic LDS that a CU holds of `fn` at once (the occupancy query, asked
// once per device, function and LDS size; beyond 48 KiB the caller has raised the function's limit first).  Negative: the query
// failed, as fail_hip reports it.  What the number permits is the caller's policy.
int resident_blocks_per_cu(const void* fn, int block, size_t lds_bytes);

// abi.hip: the pinned host word in which one unit's launches count their called-off workgroup meetings (meeting_device.h)
struct CalledOffWord {
    long long* get();              // coherent, mapped, portable; allocated and zeroed on first use; nullptr: no such memory (sticky error cleared)
    long long count() const;       // meetings called off so far
    bool changed();                // has count() moved since this was last asked?
    long long* word = nullptr;
    long long seen = 0;
};

// envs.hip: the current device's row table of the packed 2048 move (tfe_device.h), built on first use
int tfe_row_lut(const uint32_t** out);

// stoprule.hip: a check point's partial done-counts (one uint32 per wavefront / workgroup) are written in stream order
// into the slot `claim` hands out.  Their sum is published to the host by the NEXT launch on that stream: `claim` also
// returns the previous check point's counts as a `carry`, which that launch sums and publishes in its first
// workgroup, ahead of that workgroup's tables (no event, no second stream, no kernel of its own on the steps' stream).
struct StopRuleCarry {
    const uint32_t* partials;     // nullptr: nothing to carry
    int n;
    long long* host;              // {local, global, seq} in coherent pinned memory
    long long seq;
};
int stoprule_claim(PulseStopRule* h, int n_partials, uint32_t** partials_out, StopRuleCarry* carry);
int stoprule_commit(PulseStopRule* h, int n_partials, ihipStream_t* stream);

// Paired launches (lag 1 only): ONE launch runs up to two check intervals ("chunks") and decides by itself how many of
// them the rule allows.  Under the fixed-lag rule chunk c runs iff the counts of the check points c - 2 and earlier did
// not end the episode, so a launch covering the check points [a, a + k), k <= 2, needs the verdicts of a - 2 (run at
// all?) and a - 1 (run the second chunk?).  Both counts belong to launches that have COMPLETED when this one starts: its
// first workgroup sums and publishes them (the carries), the host turns them into verdicts (all-reducing over the ranks
// where there are several) and writes ONE word {launch id, skip_all, stop_mid} into pinned memory; thread 0 of the
// launch relays it into device memory, and every wavefront reads it before its first store.  No wavefront ever waits
// for another wavefront of its own launch, so the scheme needs no co-residency and works at any grid size.
struct StopRulePair {
    uint32_t* wave_done_mid;      // counts after the first chunk (nullptr when the launch covers one chunk)
    uint32_t* wave_done_fin;      // counts after the last step
    StopRuleCarry carry[2];       // check points a - 2 and a - 1, where still unpublished
    const long long* verdict_host;
    long long* verdict_dev;
    long long* verdict_err;       // pinned word a launch sets when it gave up waiting
    long long wait_ticks;         // how long the launch waits for its verdict (100 MHz ticks from its start)
    long long launch_id;
    long long first_check_point;  // a
    int n_chunks;                 // k
};
bool stoprule_pairs_supported(const PulseStopRule* h, int n_partials);
// <0: error; 0: launch; 1: the episode is already known to be over (the count a - 2 had been read earlier): do not launch
int stoprule_pair_claim(PulseStopRule* h, int n_partials, int n_chunks, StopRulePair* plan);
int stoprule_pair_commit(PulseStopRule* h, const StopRulePair* plan, int n_partials, ihipStream_t* stream);
// After the launch was enqueued: waits for the counts it carries, writes its verdict word, tells how many of its chunks run.
// *gave_up = 1: the host was too late, the launch ran nothing, the handle is back before it and pairs no more (stoprule.hip).
int stoprule_pair_verdict(PulseStopRule* h, const StopRulePair* plan, int* chunks_run, int* over, int* gave_up);

// Long launches (lag 1, a local rule, every workgroup of the launch resident at once): ONE launch covers the check points
// [a, a + m), m > 2.  Its start is the pair's protocol (carries of a - 2 and a - 1, the host's verdict word, the give-up path):
// chunks 0 and 1 run on the host's word.  Chunk r + 2 runs iff check point a + r did not end the episode, and that count
// is taken INSIDE the launch: at check point r <= m - 3 every wavefront adds {1 << 32 | its done count} to an arrival word
// (spread over n_words words with a second level; two sets, by the parity of r, zero between launches), the wavefront that
// completes the arrivals has the total, compares it with over_from and writes the verdict word {launch id << 16 | r << 8 |
// over | called off << 1} into slot r % kLongSlots of `verdicts` -- a compare-and-swap on the slot's first copy, then the
// other 63 copies.  A wavefront reads verdict r before chunk r + 2 -- and BEFORE it arrives for check point r + 1: behind an
// over or called-off word nobody arrives again, so the host is told once --; one that has waited wait_ticks calls the check point
// off with the same compare-and-swap, so exactly one word lands and every wavefront reads the same one: over or called
// off, the launch ends behind chunk r + 1, leaving the memory of a launch planned r + 2 chunks long.  Whoever wrote the
// word that settles the launch's length tells the host: {launch id << 16 | chunks run << 8 | over | called off << 1} -- an
// over or called-off word at once, a "not over" at check point m - 3 (the launch runs to its cap) otherwise.
// Early verdicts (`early`): a wavefront also LOOKS at verdict r two steps before the check point that reads it -- one load, no
// loop; a settled word is acted upon there, a pending one leaves everything to the blocking read above -- same word, same order
// of read and arrival, fewer steps that compute outputs nobody reads (poker_step.hip).
// (In the kernel's argument block as it stands here: poker_step.hip asserts the layout.)
struct StopRuleLong {
    long long* arrive;            // device, zero between launches: [2 sets][1 + kLongWords] words, one 128-byte line each; kLongWords more lines
                                  // behind them: {early looks that found their verdict settled, that found it pending} (early >= 2 only)
    long long* verdicts;         // device: [kLongSlots][64 copies], one line each
    long long* host;              // pinned: what the host learns (one word)
    uint32_t* partials;           // the ring of per-wavefront counts: check point c at partials + (c % 4) * max_partials
    uint32_t over_from;           // the smallest count that ends the episode (the host's own float comparison)
    int max_partials;
    int n_chunks;                 // m; 0: not a long launch
    int chunk_steps;
    int16_t slot0;                // a % 4
    int16_t early;                // PULSE_STOPRULE_OPT_EARLY_VERDICTS: 0 off, 1 on, 2 on + counted, 3 as 2 with every peek of an odd wavefront pending
    int skip_cp;                  // test hook: the completing wavefront of this check point does not decide (-1: none)
    int n_waves;                  // wavefronts of the launch = arrivals per check point
    int n_words;                  // first-level arrival words in use (min(kLongWords, n_waves))
    long long wait_ticks;         // how long a wavefront waits for a verdict of its own launch before it calls the check point off
};
constexpr int kLongWords = 32, kLongSlots = 4, kLongMaxChunks = 64;
// May rollout_until plan long launches of `grid` workgroups on this handle?  `resident_blocks`: the occupancy query's answer
// for the chunk kernel (asked by the caller once per handle and grid: a negative value = "ask", see stoprule_long_needs_query).
bool stoprule_long_needs_query(const PulseStopRule* h, int grid);
bool stoprule_long_launch_supported(PulseStopRule* h, int n_partials, int grid, int resident_blocks);
// after stoprule_pair_claim(.., n_chunks = m > 2, ..): the in-launch part of the plan
int stoprule_long_plan(PulseStopRule* h, const StopRulePair* plan, int n_partials, int chunk_steps, StopRuleLong* out);
// after stoprule_pair_verdict let the launch run (chunks_run == m there): how many chunks it really ran, whether the rule
// ended the episode; a called-off check point is counted and switches long launches off for the handle's life
int stoprule_long_verdict(PulseStopRule* h, const StopRulePair* plan, int* chunks_run, int* over);

}  // namespace pulse
