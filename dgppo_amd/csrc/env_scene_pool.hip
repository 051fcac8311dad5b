// The scene pool by priority (the pool of env_scene.hip's dgppo_env_scene_pool_push, with per-slot statistics): what a slot's
// replays did is folded into a score, slots are drawn in proportion to a priority of that score and of their staleness, and a push
// overwrites the slots that have stopped being useful instead of the oldest.  Everything stays on the device between rollouts.
//   dgppo_env_scene_pool_score       integer tallies per slot (atomicAdd of ints: order-free), then one lane per slot folds them
//   dgppo_env_scene_pool_draw        one workgroup: a u64 prefix sum of the integer weights, one Philox draw and one binary search per env
//   dgppo_env_scene_pool_push_evict  one workgroup: two ballot-and-prefix compactions, over the ring slots and over the envs
// The priority is formed in one place, scene_w / scene_q below; tests/scene_priority_np.py restates it.  Built with -ffp-contract=off
// like env_scene.hip: every fp32 operation here is a single IEEE operation in the order written.
#include <stdio.h>
#include "common.h"

#define SCENE_POOL_WAVES 4                               // waves of the one-workgroup kernels
#define SCENE_POOL_BLOCK (64 * SCENE_POOL_WAVES)
#define SCENE_POOL_MAX_M 65536
#define SCENE_POOL_MAX_AGE 1024
#define SCENE_MAX_AGENTS 64

// w(s) = 4 s (1 - s), clamped to [0, 1]; a NaN gives 0.  Peaks at a failure rate of one half
__device__ inline float scene_w(float s) {
  float w = (4.0f * s) * (1.0f - s);
  if (!(w >= 0.0f)) w = 0.0f;
  if (w > 1.0f) w = 1.0f;
  return w;
}
// the integer priority in [1, 65536]: never zero, so a live slot can always be drawn
__device__ inline uint32_t scene_q(float s) { return (uint32_t)(scene_w(s) * 65535.0f) + 1u; }

// every refusal names its entry point: dgppo_validate_cfg's own message does not
static int32_t pool_validate_cfg(const dgppo_env_cfg* cfg, const char* fn) {
  int32_t rc = dgppo_validate_cfg(cfg);
  if (rc) {
    char why[256];
    snprintf(why, sizeof(why), "%s", dgppo_last_error());
    dgppo_set_error("%s: %s", fn, why);
  }
  return rc;
}

// ---- dgppo_env_scene_pool_score ------------------------------------------------------------------------------------------------------
struct ScenePoolScoreArgs {
  const int32_t* scene_of;
  const int32_t* mix_flags;
  const int32_t* first;
  float* score;
  int32_t* visits;
  int32_t* last;
  int32_t* tally;
  float beta;
  int step;
  int32_t* state;
  int M, B;
};

// one thread per env: a replay is an env that was assigned a slot and whose scene was valid (an env that fell back ran a sampled
// episode); mix_flags is read only where scene_of names a slot
__global__ __launch_bounds__(SCENE_POOL_BLOCK) void env_scene_pool_tally_kernel(ScenePoolScoreArgs a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b == 0) {                                          // the fold kernel, which runs after this one, adds into them
    a.state[6] = 0;
    a.state[7] = 0;
  }
  if (b >= a.B) return;
  const int m = a.scene_of[b];
  if (m < 0 || m >= a.M) return;
  if (a.mix_flags[b] != 0) return;
  atomicAdd(&a.tally[2 * m], 1);
  if (a.first[b] >= 0) atomicAdd(&a.tally[2 * m + 1], 1);
}

// one lane per slot: the EMA, the visit count and the step of the last replay; the tally is left zero for the next call
__global__ __launch_bounds__(SCENE_POOL_BLOCK) void env_scene_pool_fold_kernel(ScenePoolScoreArgs a) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  int r = 0, f = 0;
  if (m < a.M) {
    r = a.tally[2 * m];
    f = a.tally[2 * m + 1];
    if (r > 0) {
      const float y = (float)f / (float)r;
      const float s = a.score[m];
      a.score[m] = s + a.beta * (y - s);
      a.visits[m] = (int32_t)((uint32_t)a.visits[m] + (uint32_t)r);
      a.last[m] = a.step;
      a.tally[2 * m] = 0;
      a.tally[2 * m + 1] = 0;
    }
  }
  for (int d = 32; d >= 1; d >>= 1) {
    r += __shfl_xor(r, d);
    f += __shfl_xor(f, d);
  }
  if ((threadIdx.x & 63) == 0 && r > 0) {
    atomicAdd(&a.state[6], r);
    atomicAdd(&a.state[7], f);
  }
}

extern "C" int32_t dgppo_env_scene_pool_score(const dgppo_env_cfg* cfg, const int32_t* scene_of, const int32_t* mix_flags,
                                              const int32_t* first, float* score, int32_t* visits, int32_t* last, int32_t* tally,
                                              int32_t M, float beta, int32_t step, int32_t* state, int32_t B, void* stream) {
  const char* fn = "dgppo_env_scene_pool_score";
  int32_t rc = pool_validate_cfg(cfg, fn);
  if (rc) return rc;
  DGPPO_REFUSE_VMAS(cfg, fn, "nothing (VMASReverseTransport has no scene entry point)");
  DGPPO_REQUIRE(B >= 0, "%s: B must be >= 0 (got %d)", fn, B);
  DGPPO_REQUIRE(M >= 1 && M <= SCENE_POOL_MAX_M, "%s: M must be in [1, %d] (got %d)", fn, SCENE_POOL_MAX_M, M);
  DGPPO_REQUIRE(beta > 0.0f && beta <= 1.0f, "%s: beta must be in (0, 1] (got %g)", fn, (double)beta);
  DGPPO_REQUIRE(B == 0 || (scene_of && mix_flags && first), "%s: scene_of/mix_flags/first must not be NULL", fn);
  DGPPO_REQUIRE(score && visits && last && tally && state, "%s: score/visits/last/tally/state must not be NULL", fn);
  ScenePoolScoreArgs a;
  a.scene_of = scene_of; a.mix_flags = mix_flags; a.first = first; a.score = score; a.visits = visits; a.last = last;
  a.tally = tally; a.beta = beta; a.step = step; a.state = state; a.M = M; a.B = B;
  hipLaunchKernelGGL(env_scene_pool_tally_kernel, dim3(B > 0 ? cdiv(B, SCENE_POOL_BLOCK) : 1), dim3(SCENE_POOL_BLOCK), 0,
                     (hipStream_t)stream, a);
  DGPPO_LAUNCH_CHECK();
  hipLaunchKernelGGL(env_scene_pool_fold_kernel, dim3(cdiv(M, SCENE_POOL_BLOCK)), dim3(SCENE_POOL_BLOCK), 0, (hipStream_t)stream, a);
  DGPPO_LAUNCH_CHECK();
  return 0;
}

// ---- dgppo_env_scene_pool_draw -------------------------------------------------------------------------------------------------------
struct ScenePoolDrawArgs {
  const float* score;
  const int32_t* last;
  const int32_t* state;
  uint64_t* cum;
  int M, fixed, age_cap, step;
  uint64_t seed;
  long long n_total, n_scene, lo;
  int32_t* scene_of;
  int B;
};

// inclusive prefix sum over the wave's lanes; the u64 travels as two words
__device__ inline uint64_t wave_scan_u64(uint64_t v, int lane) {
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t lo = __shfl_up((uint32_t)v, d), hi = __shfl_up((uint32_t)(v >> 32), d);
    if (lane >= d) v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}

__global__ __launch_bounds__(SCENE_POOL_BLOCK) void env_scene_pool_draw_kernel(ScenePoolDrawArgs a) {
  __shared__ uint64_t wave_sum[SCENE_POOL_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int live_end = a.fixed + a.state[1];
  uint64_t carry = 0;                                    // the weights of the chunks before this one
  for (int chunk = 0; chunk < a.M; chunk += SCENE_POOL_BLOCK) {
    const int m = chunk + tid;
    uint64_t Q = 0;
    if (m < a.M && (m < a.fixed || m < live_end)) {
      long long age = 1ll + max((long long)a.step - (long long)a.last[m], 0ll);
      if (age > a.age_cap) age = a.age_cap;
      Q = (uint64_t)scene_q(a.score[m]) * (uint64_t)age;
    }
    const uint64_t inc = wave_scan_u64(Q, lane);
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    uint64_t before = 0, total = 0;
    for (int w = 0; w < SCENE_POOL_WAVES; ++w) {
      const uint64_t s = wave_sum[w];
      if (w < wave) before += s;
      total += s;
    }
    if (m < a.M) a.cum[m] = carry + before + inc;        // the inclusive prefix sum of Q
    carry += total;
    __syncthreads();                                     // wave_sum is rewritten by the next chunk; after the last, cum is complete
  }
  const uint64_t total = carry;
  const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
  for (int b = tid; b < a.B; b += SCENE_POOL_BLOCK) {
    const long long g = a.lo + b;
    const long long k = g * a.n_scene / a.n_total;
    int32_t slot = -1;
    if ((g + 1) * a.n_scene / a.n_total > k && total != 0) {
      const Philox4 p = philox4x32_10((uint32_t)k, (uint32_t)a.step, 0u, 0u, k0, k1);
      const uint64_t u = ((uint64_t)p.v[0] << 32) | (uint64_t)p.v[1];
      const uint64_t t = __umul64hi(u, total);           // t < total = cum[M - 1]: the search below ends on a slot with Q > 0
      int lo = 0, hi = a.M - 1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.cum[mid] > t) hi = mid; else lo = mid + 1;
      }
      slot = lo;
    }
    a.scene_of[b] = slot;
  }
}

extern "C" int32_t dgppo_env_scene_pool_draw(const dgppo_env_cfg* cfg, const float* score, const int32_t* last, const int32_t* state,
                                             int32_t M, int32_t fixed, int32_t age_cap, int32_t step, uint64_t draw_seed,
                                             int64_t n_total, int64_t n_scene, int64_t lo, uint64_t* cum, int32_t* scene_of, int32_t B,
                                             void* stream) {
  const char* fn = "dgppo_env_scene_pool_draw";
  int32_t rc = pool_validate_cfg(cfg, fn);
  if (rc) return rc;
  DGPPO_REFUSE_VMAS(cfg, fn, "nothing (VMASReverseTransport has no scene entry point)");
  DGPPO_REQUIRE(B >= 0, "%s: B must be >= 0 (got %d)", fn, B);
  DGPPO_REQUIRE(M >= 1 && M <= SCENE_POOL_MAX_M, "%s: M must be in [1, %d] (got %d)", fn, SCENE_POOL_MAX_M, M);
  DGPPO_REQUIRE(fixed >= 0 && fixed < M, "%s: fixed must be in [0, M) (got %d, M %d)", fn, fixed, M);
  DGPPO_REQUIRE(age_cap >= 1 && age_cap <= SCENE_POOL_MAX_AGE, "%s: age_cap must be in [1, %d] (got %d)", fn, SCENE_POOL_MAX_AGE,
                age_cap);
  DGPPO_REQUIRE(n_total >= 1 && n_total <= 0x7fffffffll, "%s: n_total must be in [1, 2^31) (got %lld)", fn, (long long)n_total);
  DGPPO_REQUIRE(n_scene >= 0 && n_scene <= n_total, "%s: n_scene must be in [0, n_total] (got %lld, n_total %lld)", fn,
                (long long)n_scene, (long long)n_total);
  DGPPO_REQUIRE(lo >= 0 && lo + (int64_t)B <= n_total, "%s: the window [lo, lo + B) must lie in the batch (got lo %lld, B %d, n_total %lld)",
                fn, (long long)lo, B, (long long)n_total);
  DGPPO_REQUIRE(score && last && state && cum && scene_of, "%s: score/last/state/cum/scene_of must not be NULL", fn);
  if (B == 0) return 0;
  ScenePoolDrawArgs a;
  a.score = score; a.last = last; a.state = state; a.cum = cum; a.M = M; a.fixed = fixed; a.age_cap = age_cap; a.step = step;
  a.seed = draw_seed; a.n_total = n_total; a.n_scene = n_scene; a.lo = lo; a.scene_of = scene_of; a.B = B;
  hipLaunchKernelGGL(env_scene_pool_draw_kernel, dim3(1), dim3(SCENE_POOL_BLOCK), 0, (hipStream_t)stream, a);
  DGPPO_LAUNCH_CHECK();
  return 0;
}

// ---- dgppo_env_scene_pool_push_evict -------------------------------------------------------------------------------------------------
// Phase 1 ranks the evictable filled ring positions in ring order from head (a ballot per wave, a prefix over the waves in LDS, chunks of
// the block size over R) and lists them in `order`; phase 2 ranks the taken envs as dgppo_env_scene_pool_push does and sends rank r to
// the r-th empty position, then to order[r - empties].  The ranks are distinct, so are the slots, and no atomic decides anything.
struct ScenePoolPushArgs {
  const int32_t* first;
  const int32_t* flags;
  const uint32_t* agent_t;
  const uint32_t* goal_t;
  const uint32_t* obst_t;
  uint32_t* pool_agent;
  uint32_t* pool_goal;
  uint32_t* pool_obst;
  int words_agent, words_goal, words_obst;               // per row
  float* score;
  int32_t* visits;
  int32_t* last;
  int32_t* order;
  int M, fixed, min_visits, step;
  float evict_w;
  int32_t* state;
  int32_t* slot_of;
  int B;
};

__global__ __launch_bounds__(SCENE_POOL_BLOCK) void env_scene_pool_push_evict_kernel(ScenePoolPushArgs a) {
  __shared__ int wave_count[SCENE_POOL_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int R = a.M - a.fixed;
  // read before the first barrier, written after the last; clamped, so that no state word can send a row outside the ring
  const int head = ((a.state[0] % R) + R) % R, filled = min(max(a.state[1], 0), R), pushed = a.state[2];
  const int n_empty = R - filled;
  int n_evict = 0;                                       // evictable positions of the chunks before this one
  for (int chunk = 0; chunk < R; chunk += SCENE_POOL_BLOCK) {
    const int i = chunk + tid;
    const int pos = i < R ? (head + i) % R : 0;
    const int m = a.fixed + pos;
    const bool ev = i < R && pos < filled && a.visits[m] >= a.min_visits && scene_w(a.score[m]) <= a.evict_w;
    const unsigned long long ballot = __ballot(ev);
    if (lane == 0) wave_count[wave] = __popcll(ballot);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < SCENE_POOL_WAVES; ++w) {
      const int cnt = wave_count[w];
      if (w < wave) before += cnt;
      total += cnt;
    }
    if (ev) a.order[n_evict + before + __popcll(ballot & ((1ull << lane) - 1ull))] = pos;
    n_evict += total;
    __syncthreads();                                     // wave_count is rewritten; after the last chunk, order is complete
  }
  int base = 0;                                          // taken envs of the chunks before this one
  for (int chunk = 0; chunk < a.B; chunk += SCENE_POOL_BLOCK) {
    const int b = chunk + tid;
    const bool taken = b < a.B && a.first[b] >= 1 && a.flags[b] == 0;
    const unsigned long long ballot = __ballot(taken);
    if (lane == 0) wave_count[wave] = __popcll(ballot);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < SCENE_POOL_WAVES; ++w) {
      const int cnt = wave_count[w];
      if (w < wave) before += cnt;
      total += cnt;
    }
    const int r = base + before + __popcll(ballot & ((1ull << lane) - 1ull));
    int slot = -1;
    if (taken && r < n_empty) slot = a.fixed + filled + r;
    else if (taken && r - n_empty < n_evict) slot = a.fixed + a.order[r - n_empty];
    if (b < a.B && a.slot_of) a.slot_of[b] = slot;
    if (slot >= 0) {
      a.score[slot] = 0.5f;
      a.visits[slot] = 0;
      a.last[slot] = a.step;
    }
    unsigned long long todo = __ballot(slot >= 0);
    while (todo) {                                       // wave-uniform: one taken env of this wave per trip
      const int k = __ffsll((long long)todo) - 1;
      todo &= todo - 1ull;
      const size_t src = (size_t)(chunk + wave * 64 + k), dst = (size_t)__shfl(slot, k);
      for (int i = lane; i < a.words_agent; i += 64) a.pool_agent[dst * a.words_agent + i] = a.agent_t[src * a.words_agent + i];
      for (int i = lane; i < a.words_goal; i += 64) a.pool_goal[dst * a.words_goal + i] = a.goal_t[src * a.words_goal + i];
      for (int i = lane; i < a.words_obst; i += 64) a.pool_obst[dst * a.words_obst + i] = a.obst_t[src * a.words_obst + i];
    }
    base += total;
    __syncthreads();                                     // wave_count is rewritten by the next chunk
  }
  if (tid == 0) {
    const int to_empty = min(base, n_empty);
    const int evicted = min(base - to_empty, n_evict);
    if (evicted > 0) a.state[0] = (a.order[evicted - 1] + 1) % R;
    a.state[1] = filled + to_empty;
    a.state[2] = (int32_t)((uint32_t)pushed + (uint32_t)(to_empty + evicted));
    a.state[3] = base;
    a.state[4] = evicted;
    a.state[5] = base - to_empty - evicted;
  }
}

extern "C" int32_t dgppo_env_scene_pool_push_evict(const dgppo_env_cfg* cfg, const int32_t* first, const int32_t* flags,
                                                   const float* agent_t, const float* goal_t, const float* obst_t, float* pool_agent,
                                                   float* pool_goal, float* pool_obst, float* score, int32_t* visits, int32_t* last,
                                                   int32_t* order, int32_t M, int32_t fixed, int32_t min_visits, float evict_w,
                                                   int32_t step, int32_t* state, int32_t* slot_of, int32_t B, void* stream) {
  const char* fn = "dgppo_env_scene_pool_push_evict";
  int32_t rc = pool_validate_cfg(cfg, fn);
  if (rc) return rc;
  DGPPO_REFUSE_VMAS(cfg, fn, "nothing (VMASReverseTransport has no scene entry point)");
  DGPPO_REQUIRE(B >= 0, "%s: B must be >= 0 (got %d)", fn, B);
  DGPPO_REQUIRE(M >= 1 && M <= SCENE_POOL_MAX_M, "%s: M must be in [1, %d] (got %d)", fn, SCENE_POOL_MAX_M, M);
  DGPPO_REQUIRE(fixed >= 0 && fixed < M, "%s: fixed must be in [0, M) (got %d, M %d)", fn, fixed, M);
  DGPPO_REQUIRE(min_visits >= 0, "%s: min_visits must be >= 0 (got %d)", fn, min_visits);
  DGPPO_REQUIRE(evict_w >= 0.0f && evict_w <= 1.0f, "%s: evict_w must be in [0, 1] (got %g)", fn, (double)evict_w);
  DGPPO_REQUIRE(B == 0 || (first && flags && agent_t && goal_t), "%s: first/flags/agent_t/goal_t must not be NULL", fn);
  DGPPO_REQUIRE(pool_agent && pool_goal && state, "%s: pool_agent/pool_goal/state must not be NULL", fn);
  DGPPO_REQUIRE(score && visits && last && order, "%s: score/visits/last/order must not be NULL", fn);
  DGPPO_REQUIRE(B == 0 || (cfg->n_obs == 0) == (obst_t == nullptr), "%s: obst_t must be NULL exactly when n_obs == 0", fn);
  DGPPO_REQUIRE((cfg->n_obs == 0) == (pool_obst == nullptr), "%s: pool_obst must be NULL exactly when n_obs == 0", fn);
  DGPPO_REQUIRE(cfg->n_agents <= SCENE_MAX_AGENTS, "%s supports at most %d agents", fn, SCENE_MAX_AGENTS);
  ScenePoolPushArgs a;
  a.first = first; a.flags = flags; a.agent_t = (const uint32_t*)agent_t; a.goal_t = (const uint32_t*)goal_t;
  a.obst_t = (const uint32_t*)obst_t; a.pool_agent = (uint32_t*)pool_agent; a.pool_goal = (uint32_t*)pool_goal;
  a.pool_obst = (uint32_t*)pool_obst;
  a.words_agent = cfg->n_agents * cfg->state_dim; a.words_goal = cfg->n_goals * cfg->state_dim;
  a.words_obst = cfg->n_obs * (cfg_is_lidar(*cfg) ? 5 : 2);
  a.score = score; a.visits = visits; a.last = last; a.order = order; a.M = M; a.fixed = fixed; a.min_visits = min_visits;
  a.step = step; a.evict_w = evict_w; a.state = state; a.slot_of = slot_of; a.B = B;
  hipLaunchKernelGGL(env_scene_pool_push_evict_kernel, dim3(1), dim3(SCENE_POOL_BLOCK), 0, (hipStream_t)stream, a);
  DGPPO_LAUNCH_CHECK();
  return 0;
}
