// poker_rollout.hip -- the host side of a hold'em roll-out: the HIP-event timer, n steps enqueued by one native call (pulse_poker_rollout)
// and the trainer's episode loop with the stop rule in it (pulse_poker_rollout_until).  The launches are poker_step.hip's (poker_launch.h).
#include <hip/hip_runtime.h>

#include "poker_device.h"
#include "poker_launch.h"

using pulse::ChunkArgs;
using pulse::PolicyArgs;

// HIP-event timer owned by the caller: brackets whole roll-out calls on their launch stream
struct PulseTimer {
    static constexpr int kMax = 4096;
    hipEvent_t start[kMax], stop[kMax];
    int launches[kMax], steps[kMax];
    int created = 0, used = 0;
    long long calls = 0;                  // chunks seen by pulse_poker_rollout_until (a bracket opens every time_every-th)
    bool open = false;                    // a bracket is open: start recorded, stop not yet
    int open_launches = 0, open_steps = 0;
};

namespace {
constexpr int kTimedSpan = 8;             // consecutive chunks per event pair (an episode has at most eight): the pair's own queue time is shared
int timer_begin(PulseTimer* tm, hipStream_t st) {
    if (tm->used >= PulseTimer::kMax) return 0;
    if (tm->used >= tm->created) {
        if (hipEventCreate(&tm->start[tm->created]) != hipSuccess || hipEventCreate(&tm->stop[tm->created]) != hipSuccess)
            return pulse::fail(PULSE_ENODEVICE, "roll-out timer: hipEventCreate failed");
        ++tm->created;
    }
    const hipError_t e = hipEventRecord(tm->start[tm->used], st);
    if (e != hipSuccess) return pulse::fail_hip((int)e, "roll-out timer: hipEventRecord");
    tm->open = true; tm->open_launches = 0; tm->open_steps = 0;
    return 0;
}
void timer_end(PulseTimer* tm, hipStream_t st) {
    (void)hipEventRecord(tm->stop[tm->used], st);
    tm->launches[tm->used] = tm->open_launches; tm->steps[tm->used] = tm->open_steps; ++tm->used;
    tm->open = false;
}
// one chunk launch of a paired sequence (pulse_internal.h: StopRulePair)
void launch_pair(const PulsePokerView& v_even, const PulsePokerView& v_odd, uint64_t packed, uint64_t seed, uint64_t step_counter0,
                 uint64_t table_id0, int64_t* actions, float* rewards_even, float* rewards_odd, int n_steps, int chunk_steps,
                 const pulse::StopRulePair& plan, const pulse::StopRuleLong* lng, hipStream_t st) {
    PolicyArgs pa(packed, seed, step_counter0, table_id0);
    if (lng) pa.lng = *lng;
    pa.wave_done = plan.wave_done_fin;
    pa.carry[0] = plan.carry[0]; pa.carry[1] = plan.carry[1];
    if (pa.carry[0].n == 0 && pa.carry[1].n > 0) { pa.carry[0] = pa.carry[1]; pa.carry[1].n = 0; }      // (cannot happen: carries are filled in order; kept for safety)
    pa.wave_done_mid = plan.wave_done_mid; pa.mid_step = plan.n_chunks >= 2 ? chunk_steps : 0;
    pa.verdict_host = plan.verdict_host; pa.verdict_dev = plan.verdict_dev; pa.verdict_id = plan.launch_id; pa.verdict_err = plan.verdict_err;
    pa.verdict_ticks = plan.wait_ticks;
    pulse::launch_chunk(v_even, actions, rewards_even, pa, ChunkArgs{v_odd.obs, rewards_odd, n_steps}, st);
}
}  // namespace

extern "C" {

int pulse_timer_create(void** out) {
    if (!out) return pulse::fail(PULSE_EINVAL, "pulse_timer_create: null argument");
    *out = new PulseTimer();
    return 0;
}

int pulse_timer_destroy(void* timer) {
    PulseTimer* tm = static_cast<PulseTimer*>(timer);
    if (!tm) return 0;
    for (int i = 0; i < tm->created; ++i) { (void)hipEventDestroy(tm->start[i]); (void)hipEventDestroy(tm->stop[i]); }
    delete tm;
    return 0;
}

int pulse_timer_collect(void* timer, float* sum_ms, int32_t* n_launches, int64_t* n_steps) {
    PulseTimer* tm = static_cast<PulseTimer*>(timer);
    if (!tm || !sum_ms || !n_launches || !n_steps) return pulse::fail(PULSE_EINVAL, "pulse_timer_collect: null argument");
    float total = 0.0f; int launches = 0; long long steps = 0;
    for (int i = 0; i < tm->used; ++i) {
        float ms = 0.0f;
        const hipError_t e = hipEventElapsedTime(&ms, tm->start[i], tm->stop[i]);
        if (e != hipSuccess) return pulse::fail_hip((int)e, "pulse_timer_collect (call it after a stream sync)");
        total += ms; launches += tm->launches[i]; steps += tm->steps[i];
    }
    *sum_ms = total; *n_launches = launches; *n_steps = steps;
    tm->used = 0;
    return 0;
}

int pulse_poker_rollout(const PulsePokerView* v_even, const PulsePokerView* v_odd, const uint8_t* agent_types,
                        uint64_t seed, uint64_t step_counter0, uint64_t table_id0, int64_t* actions, float* rewards_even,
                        float* rewards_odd, int32_t n_steps, void* timer, void* stoprule, void* stream) {
    if (int rc = pulse::check_view(v_even, "pulse_poker_rollout")) return rc;
    if (int rc = pulse::check_view(v_odd, "pulse_poker_rollout")) return rc;
    if (!actions || !rewards_even || !rewards_odd || !agent_types || n_steps < 0)
        return pulse::fail(PULSE_EINVAL, "pulse_poker_rollout: bad argument");
    if (v_even->is_done != v_odd->is_done_out || v_even->is_done_out != v_odd->is_done || v_even->n_games != v_odd->n_games)
        return pulse::fail(PULSE_EINVAL, "pulse_poker_rollout: v_odd must be v_even with is_done / is_done_out swapped");
    if (v_even->n_games == 0 || n_steps == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const uint64_t packed = pulse::pack_types(agent_types, v_even->n_players);
    // one step is what the single-step kernel is for (15.4 vs 18.1 us at 65,536 tables: no LDS staging to amortise)
    const bool chunk = !(v_even->flags & PULSE_VIEW_NO_CHUNK) && n_steps > 1;
    PulseTimer* tm = static_cast<PulseTimer*>(timer);
    const bool timed = tm && !tm->open && tm->used < PulseTimer::kMax;
    if (timed) if (int rc = timer_begin(tm, st)) return rc;
    PulseStopRule* rule = static_cast<PulseStopRule*>(stoprule);
    const int n_waves = pulse::launch_waves(v_even->n_games, pulse::lanes_for(*v_even, chunk));
    PolicyArgs pa(packed, seed, step_counter0, table_id0);      // of the chunk / of the first step: it carries the previous check point
    if (rule) if (int rc = pulse::stoprule_claim(rule, n_waves, &pa.wave_done, &pa.carry[0])) return rc;
    if (chunk) {
        // (streaming, non-temporal observation stores were measured: -1 % per chunk up to 262,144 tables, +4 % at 1 M --
        // and +50 % fabric write traffic, since ordinary stores to the two ping-pong blocks are largely absorbed by the
        // caches.  Not used.)
        pulse::launch_chunk(*v_even, actions, rewards_even, pa, ChunkArgs{v_odd->obs, rewards_odd, n_steps}, st);
    } else {
        uint32_t* const wave_done = pa.wave_done;            // the last step counts the done tables
        for (int i = 0; i < n_steps; ++i) {
            pa.step_counter = step_counter0 + (uint64_t)i;
            pa.wave_done = i == n_steps - 1 ? wave_done : nullptr;
            pulse::launch_policy_step((i & 1) ? *v_odd : *v_even, actions, (i & 1) ? rewards_odd : rewards_even, pa, st);
            pa.carry[0] = pulse::StopRuleCarry{};
        }
    }
    if (timed) { tm->open_launches = chunk ? 1 : n_steps; tm->open_steps = n_steps; timer_end(tm, st); }
    if (int rc = pulse::finish_launch("pulse_poker_rollout")) return rc;
    if (rule) return pulse::stoprule_commit(rule, n_waves, st);
    return 0;
}

int pulse_poker_rollout_until(const PulsePokerView* v_even, const PulsePokerView* v_odd, const uint8_t* agent_types,
                              uint64_t seed, uint64_t step_counter0, uint64_t table_id0, int64_t* actions, float* rewards_even,
                              float* rewards_odd, int32_t chunk_steps, int32_t max_steps, void* timer, int32_t time_every,
                              void* stoprule, void* stream, int32_t* steps_done, int32_t* over) {
    if (!steps_done || !over || chunk_steps <= 0 || max_steps < 0 || !stoprule)
        return pulse::fail(PULSE_EINVAL, "pulse_poker_rollout_until: bad argument");
    if (int rc = pulse::check_view(v_even, "pulse_poker_rollout_until")) return rc;
    if (int rc = pulse::check_view(v_odd, "pulse_poker_rollout_until")) return rc;
    if (!actions || !rewards_even || !rewards_odd || !agent_types) return pulse::fail(PULSE_EINVAL, "pulse_poker_rollout_until: null argument");
    PulseTimer* tm = static_cast<PulseTimer*>(timer);
    hipStream_t st = (hipStream_t)stream;
    const bool per_step = (v_even->flags & PULSE_VIEW_NO_CHUNK) != 0;
    PulseStopRule* rule = static_cast<PulseStopRule*>(stoprule);
    int done = 0, parity = 0, verdict = 0;
    bool fell_back = false;
    // ---- paired launches: with the lag-1 rule ONE launch runs up to two check intervals and takes the rule's verdicts on
    // the two check points before them itself (pulse_internal.h: StopRulePair) -- half as many state load bursts and
    // store tails per episode, the same episodes step for step.  (PULSE_VIEW_NO_PAIRS / lag 0 / lag 2 / RCCL: one check
    // interval per launch, below.)
    const int n_waves_chunk = pulse::launch_waves(v_even->n_games, pulse::lanes_for(*v_even, true));
    const bool pairs = !per_step && !(v_even->flags & PULSE_VIEW_NO_PAIRS) && chunk_steps > 1 && v_even->n_games > 0 &&
                       pulse::stoprule_pairs_supported(rule, n_waves_chunk);
    if (pairs) {
        const uint64_t packed = pulse::pack_types(agent_types, v_even->n_players);
        const int grid = pulse::chunk_grid(*v_even);
        while (done < max_steps && !verdict) {
            const int left = max_steps - done;
            // More than one pair's worth of full check intervals left: ONE launch for all the intervals the pairs would cover,
            // where the handle and the grid allow it (pulse_internal.h: StopRuleLong); otherwise pairs, exactly as before.
            // What is then left of the call (less than two intervals) runs with one interval per launch as it always has,
            // so a call returns the same (steps, over) as with pairs: a launch that runs all its chunks reports `over` with
            // the NEXT launch, and whether a call's last launch is such a one must not depend on the mode.
            const int m = 2 * (left / (2 * chunk_steps));
            bool lng = false;
            if (m > 2 && m <= pulse::kLongMaxChunks && !(v_even->flags & PULSE_VIEW_NO_LONG_LAUNCHES)) {
                int resident = 0;
                if (pulse::stoprule_long_needs_query(rule, grid)) {
                    resident = pulse::chunk_resident_blocks(*v_even, v_odd->obs, nullptr);
                    if (resident < 0) return resident;
                }
                lng = pulse::stoprule_long_launch_supported(rule, n_waves_chunk, grid, resident);
            }
            const int k = lng ? m : left >= 2 * chunk_steps ? 2 : 1;
            const int n = lng ? m * chunk_steps : k == 2 ? 2 * chunk_steps : (left < chunk_steps ? left : chunk_steps);
            pulse::StopRulePair plan;
            const int c = pulse::stoprule_pair_claim(rule, n_waves_chunk, k, &plan);
            if (c < 0) return c;
            if (c == 1) { verdict = 1; break; }
            if (tm && time_every > 0 && !tm->open && (tm->calls % time_every) == 0) if (int rc = timer_begin(tm, st)) return rc;
            if (tm) ++tm->calls;
            pulse::StopRuleLong in_launch{};
            if (lng) if (int rc = pulse::stoprule_long_plan(rule, &plan, n_waves_chunk, chunk_steps, &in_launch)) return rc;
            launch_pair(parity ? *v_odd : *v_even, parity ? *v_even : *v_odd, packed, seed, step_counter0 + (uint64_t)done, table_id0, actions,
                        parity ? rewards_odd : rewards_even, parity ? rewards_even : rewards_odd, n, chunk_steps, plan, lng ? &in_launch : nullptr, st);
            if (int rc = pulse::finish_launch("pulse_poker_rollout_until")) return rc;
            if (int rc = pulse::stoprule_pair_commit(rule, &plan, n_waves_chunk, st)) return rc;
            int chunks_run = 0, gave_up = 0;
            if (int rc = pulse::stoprule_pair_verdict(rule, &plan, &chunks_run, &verdict, &gave_up)) return rc;
            if (gave_up) {                  // the host was too late for this launch: it ran nothing; the rule pairs no more
                fell_back = !verdict;       // (unless the episode had ended before it anyway) its steps run below, one check interval per launch
                break;
            }
            // a long launch the host's word let run: how far it went is its own news
            if (lng && chunks_run == k) if (int rc = pulse::stoprule_long_verdict(rule, &plan, &chunks_run, &verdict)) return rc;
            const int ran = chunks_run == k ? n : chunks_run * chunk_steps;
            done += ran; parity ^= ran & 1;
            if (tm && tm->open) {
                tm->open_launches += 1; tm->open_steps += ran;
                if (tm->open_launches >= kTimedSpan) timer_end(tm, st);
            }
        }
        if (!fell_back) {
            if (tm && tm->open) timer_end(tm, st);
            *steps_done = done; *over = verdict;
            return 0;
        }
    }
    while (done < max_steps && !verdict) {
        const int n = chunk_steps < max_steps - done ? chunk_steps : max_steps - done;
        // an event pair brackets kTimedSpan consecutive chunks, every time_every-th chunk opens one
        if (tm && time_every > 0 && !tm->open && (tm->calls % time_every) == 0) if (int rc = timer_begin(tm, st)) return rc;
        if (tm) ++tm->calls;
        // after an odd number of steps the roles of the two views (and reward buffers) are swapped
        if (int rc = pulse_poker_rollout(parity ? v_odd : v_even, parity ? v_even : v_odd, agent_types, seed, step_counter0 + (uint64_t)done,
                                         table_id0, actions, parity ? rewards_odd : rewards_even, parity ? rewards_even : rewards_odd, n,
                                         nullptr, stoprule, stream)) return rc;
        done += n; parity ^= n & 1;
        if (tm && tm->open) {
            tm->open_launches += per_step ? n : 1; tm->open_steps += n;
            if (tm->open_launches >= (per_step ? kTimedSpan * chunk_steps : kTimedSpan)) timer_end(tm, st);
        }
        if (int rc = pulse_stoprule_decide(stoprule, &verdict)) return rc;
    }
    if (tm && tm->open) timer_end(tm, st);            // the episode ended inside a bracket: it covers what ran
    *steps_done = done; *over = verdict;
    return 0;
}

}  // extern "C"
