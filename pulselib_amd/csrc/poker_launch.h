// poker_launch.h -- the step kernel's launch arguments and the launchers of poker_step.hip that the roll-out drivers
// (poker_rollout.hip) call.  Not part of the ABI.
#pragma once
#include "pulse_internal.h"

namespace pulse {

// The fused policy's arguments: a kernel argument of every step launch (poker_step.hip asserts the layout).
struct PolicyArgs {
    uint64_t types_packed = 0, seed = 0, step_counter = 0, table_id0 = 0;
    uint32_t* wave_done = nullptr;         // nullptr, or one word per wavefront of the launch: tables done after the last step
    // the PREVIOUS check points' wavefront counts, summed and published to the host by workgroup 0 of this launch, before its
    // own tables: [0] alone for an ordinary launch, [0] and [1] for a paired one (StopRulePair); filled in order
    StopRuleCarry carry[2] = {};
    // paired launches: the counts after the launch's first chunk, and the verdict word
    // {launch id << 8 | skip_all | stop_mid << 1 | error << 7} the host answers the carries with
    uint32_t* wave_done_mid = nullptr; int mid_step = 0;
    const long long* verdict_host = nullptr; long long* verdict_dev = nullptr; long long verdict_id = 0;
    long long* verdict_err = nullptr;      // pinned: set by a launch that gave up waiting for its verdict (the host then runs its steps unpaired)
    long long verdict_ticks = 0;           // ticks of the 100 MHz wall clock thread 0 waits for the word: a launch never waits for a dead host for ever
    // long launches (pulse_internal.h: StopRuleLong): n_chunks > 2 check intervals, the verdicts from the third chunk on taken in-launch
    StopRuleLong lng = {};
    PolicyArgs() = default;
    PolicyArgs(uint64_t types, uint64_t seed_, uint64_t step, uint64_t id0) : types_packed(types), seed(seed_), step_counter(step), table_id0(id0) {}
};
struct ChunkArgs { float* obs_odd = nullptr; float* rewards_odd = nullptr; int n_steps = 1; };   // chunk launches only: the odd steps' output buffers, the number of steps

int lanes_for(const PulsePokerView& v, bool chunk);         // lanes per table of a single-step / chunk launch on this view
inline int launch_waves(int n_games, int lpt) { return (int)(((long long)n_games * lpt + 63) / 64); }   // wavefronts of that launch
// one fused policy + step launch / one chunk of ca.n_steps of them (errors: pulse::finish_launch)
void launch_policy_step(const PulsePokerView& v, int64_t* actions, float* rewards, const PolicyArgs& pa, ihipStream_t* st);
void launch_chunk(const PulsePokerView& v, int64_t* actions, float* rewards_even, const PolicyArgs& pa, const ChunkArgs& ca, ihipStream_t* st);
// what hipOccupancyMaxActiveBlocksPerMultiprocessor answers for the chunk-kernel instantiation launch_chunk would take on this view, with its
// dynamic LDS size (< 0: the query failed, error recorded); *grid = workgroups of that launch
int chunk_resident_blocks(const PulsePokerView& v, const float* obs_odd, int* grid);
int chunk_grid(const PulsePokerView& v);                    // workgroups of a chunk launch on this view

}  // namespace pulse
