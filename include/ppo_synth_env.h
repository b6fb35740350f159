/*
 * ppo_synth_env.h — device-resident synthetic HalfCheetah-shaped vector env (bench / test env).
 *
 * NOT part of the hot path: it stands in for the MuJoCo envs behind the gymcpp boundary
 * (libs/gymcpp/mujoco/half_cheetah_v5.h is unbuildable here — no libmujoco) so the GPU path can be
 * measured with inputs resident in HBM. Semantics follow SeqVectorEnv (libs/gymcpp/gym.h:131-163:
 * clip_actions, next-step autoreset with reward 0 / done 0 on the reset step, reset(seed + i))
 * wrapped in RecordEpisodeStatistics (libs/gymcpp/wrappers/common.h:48-65). Dynamics (the arithmetic
 * of include/ppo_cheetah.h, shared with the host SyntheticCheetah of
 * ppo.cpp_amd/gymcpp/synthetic_cheetah.h; bit for bit also the oracle's own restatement in oracle/):
 *   q'_i = fma(0.9, q_i, fma(0.1, a_{i mod A}, 0.05 * q_{(i+1) mod O}))
 *   r    = (q'_0 - q_0) / 0.05 - sum_k (0.1 a_k) a_k ;  truncation after 1000 steps, never terminates
 *
 * A second env kind, PSYN_PENDULUM (psyn_create_env("Pendulum-v1")), is a real task: Gymnasium's
 * Pendulum-v1 (O = 3, A = 1, torque in [-2, 2], truncation after 200 steps, never terminates), with
 * the arithmetic of include/ppo_pendulum.h — bit for bit the host env ppo.cpp_amd/gymcpp/pendulum.h.
 * The vector-env semantics, the episode statistics and the wrapper chain are the same for both kinds.
 * Its state q [E, 3] holds theta, thetadot and one unused slot. The dynamics clip the torque to
 * [-2, 2] themselves, whatever psyn_set_action_space says. Not covered for this kind: the VALU
 * rollout kernel (rollout_kernel=valu is refused).
 *
 * A third kind, PSYN_CARTPOLE (psyn_create_env("CartPoleContinuous-v1")), is the first whose episodes
 * terminate: Gymnasium's CartPole-v1 with the force 10 * clip(a, -1, 1) from one continuous action
 * (O = 4: x, xdot, theta, thetadot, raw; A = 1; reward 1 per step; termination when |x| > 2.4 or
 * |theta| > 12 degrees; truncation after 500 steps), with the arithmetic of include/ppo_cartpole.h —
 * bit for bit the host env ppo.cpp_amd/gymcpp/cartpole.h. Its state q [E, 4] is the observation. The
 * step's termination flag reaches NormalizeReward (the return accumulator restarts after a
 * termination, not after a truncation); done = terminated or truncated, and psyn_step still returns
 * done only. Episodes end on any step, on different steps in different envs. rollout_kernel=valu is
 * refused for this kind as well.
 *
 * A fourth kind, PSYN_REACHER (psyn_create_env("ReacherPlanar-v0")), is the first real task with a
 * two-dimensional action: a two-link planar arm, O = 10, A = 2, action space [-1, 1] per dimension,
 * truncation after 50 steps, never terminates. It is not MuJoCo's Reacher: it takes Gymnasium
 * Reacher-v5's task definition (observation layout, reward, goal distribution, truncation, action
 * space) and puts the textbook two-link manipulator equations under it, with the arithmetic of
 * include/ppo_reacher.h — bit for bit the host env ppo.cpp_amd/gymcpp/reacher.h. Its state q [E, 10]
 * holds q1, q2, q1dot, q2dot, gx, gy and four unused slots. The goal (gx, gy) is env state that no step
 * touches: it survives every step and is redrawn at every autoreset. The dynamics clip both actions to
 * [-1, 1] themselves; the termination flag passed to the wrapper chain is always 0. Not covered for
 * this kind: the VALU rollout kernel (rollout_kernel=valu is refused).
 *
 * A fifth kind, PSYN_QUADROTOR (psyn_create_env("QuadrotorHover-v0")), is the first real task wider
 * than one 16-wide input tile: a rigid-body quadrotor hovering at the origin, O = 18, A = 4, action
 * space [-1, 1] per dimension, termination when |p|^2 > 9, truncation after 500 steps. It is this
 * project's own task over the textbook Newton-Euler equations, not a simulator's quadrotor, with the
 * arithmetic of include/ppo_quadrotor.h — bit for bit the host env ppo.cpp_amd/gymcpp/quadrotor.h.
 * Its state q [E, 18] holds p, v, the unit quaternion (w, x, y, z), omega and five unused slots. The
 * dynamics clip the four actions to [-1, 1] themselves; the termination flag reaches the wrapper
 * chain as CartPole's does. Not covered for this kind: the VALU rollout kernel (rollout_kernel=valu
 * is refused).
 *
 * A sixth kind, PSYN_ACROBOT (psyn_create_env("AcrobotContinuous-v1")), is the first whose step is a
 * multi-stage integrator: Gymnasium's Acrobot-v1 ("book" dynamics, one RK4 step of 0.2 s per env step)
 * with the torque clip(a, -1, 1) from one continuous action (O = 6: cos / sin of both angles and both
 * speeds; A = 1; reward -1 per step and 0 on the terminating step; termination when the tip is above
 * the bar, -cos theta1 - cos(theta1 + theta2) > 1; truncation after 500 steps), with the arithmetic of
 * include/ppo_acrobot.h — bit for bit the host env ppo.cpp_amd/gymcpp/acrobot.h. Its state q [E, 6]
 * holds theta1, theta2, theta1dot, theta2dot and two unused slots. Termination here is success: a
 * shorter episode is the better one, and the termination flag reaches the wrapper chain as
 * CartPole's does. rollout_kernel=valu is refused for this kind as well.
 */
#ifndef PPO_SYNTH_ENV_H
#define PPO_SYNTH_ENV_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct psyn_env psyn_t;

int psyn_create(int num_envs, int obs_dim, int act_dim, psyn_t** out);
/* The env kinds. psyn_create gives PSYN_CHEETAH at any (obs_dim, act_dim). */
enum { PSYN_CHEETAH = 0, PSYN_PENDULUM = 1, PSYN_CARTPOLE = 2, PSYN_REACHER = 3, PSYN_QUADROTOR = 4, PSYN_ACROBOT = 5 };
/* By env id: "Pendulum-v1" (PSYN_PENDULUM: O = 3, A = 1, action space [-2, 2]),
 * "CartPoleContinuous-v1" (PSYN_CARTPOLE: O = 4, A = 1, action space [-1, 1]),
 * "ReacherPlanar-v0" (PSYN_REACHER: O = 10, A = 2, action space [-1, 1]^2),
 * "QuadrotorHover-v0" (PSYN_QUADROTOR: O = 18, A = 4, action space [-1, 1]^4),
 * "AcrobotContinuous-v1" (PSYN_ACROBOT: O = 6, A = 1, action space [-1, 1]) or
 * "SyntheticCheetah-v0" (the env of psyn_create(num_envs, 17, 6)). Any other id, a NULL argument or
 * num_envs <= 0 is refused (-1, ppo_last_error lists the ids) before any HIP call. */
int psyn_create_env(const char* env_id, int num_envs, psyn_t** out);
/* kind, dims and the truncation step count (1000 | 200 | 500 | 50); any output may be NULL */
int psyn_env_info(const psyn_t* env, int* kind, int* obs_dim, int* act_dim, int* max_steps);
int psyn_destroy(psyn_t* env);
/* reset(seed + i) for every env; writes obs [E,O] and done [E] (= 0) */
int psyn_reset(psyn_t* env, int seed, float* obs_dev, float* done_dev, void* stream);
/* The env's action space (default [-1, 1]); ppo_rollout_synth clips actions to it (clip_actions,
 * gym.h:141-144), e.g. Humanoid-v4's [-0.4, 0.4] (libs/gymcpp/mujoco/humanoid_v4.h:29-30). */
int psyn_set_action_space(psyn_t* env, float lo, float hi);
int psyn_action_space(const psyn_t* env, float* lo, float* hi);
/* one SeqVectorEnv step on envs [env_begin, env_end); actions are clipped to [lo, hi] */
int psyn_step(psyn_t* env, int env_begin, int env_end, const float* action_dev, float lo, float hi,
              float* obs_dev, float* reward_dev, float* done_dev, void* stream);
/* sums of finished-episode returns / lengths / counts since the last call (host floats) */
int psyn_episode_stats(psyn_t* env, float* sum_return, float* sum_length, float* count);
/* the same without a device-wide sync: _begin enqueues the read-out (and the reset of the sums)
 * on `stream`; _end waits for that read-out only and returns the sums (same values as above) */
int psyn_episode_stats_begin(psyn_t* env, void* stream);
int psyn_episode_stats_end(psyn_t* env, float* sum_return, float* sum_length, float* count);

/* Device-resident rollout driver: num_steps x {ppo_rollout_act, psyn_step, ppo_rollout_reward} on
 * the context stream (ppo_continuous_action.cpp:387-434 with this env behind the boundary).
 * act_scratch [E*A] and rew_scratch [E] are caller-provided device buffers. */
struct ppo_ctx;
int ppo_rollout_synth(struct ppo_ctx* ctx, psyn_t* env, float* next_obs_dev, float* next_done_dev,
                      float* act_scratch_dev, float* rew_scratch_dev);
/* How ppo_rollout_synth runs the T steps: PPO_ROLLOUT_AUTO (default) uses one persistent launch
 * (actor weights resident in registers, the env step and the PPO wrapper chain fused in; then the
 * critic over all stored observations) for the agent shapes the trainers build (AC agent H = 256
 * without wrappers, PPO agent H = 64), and per-step launches otherwise; PPO_ROLLOUT_PER_STEP always
 * launches per step. The persistent kernels run the arithmetic of the per-step act kernels k_act3
 * (AC) and k_act4 (PPO; the per-step default at O >= 112, option act_kernel=4 otherwise): storage,
 * env state and episode statistics are then bitwise identical. */
enum { PPO_ROLLOUT_AUTO = 0, PPO_ROLLOUT_PER_STEP = 1 };
int ppo_set_rollout_mode(struct ppo_ctx* ctx, int mode);

/* Policy evaluation on the device env: "what return does this policy get"
 * (ac_ppo_continuous_action.cpp:965-1001 with num_eval_envs = 1; ppo_continuous_action.cpp:589-626
 * with num_eval_envs = E).
 *
 * psyn_reset(env, eval_seed), then the envs [0, num_eval_envs) each run their own trajectory: act
 * (Beta mean / roach / sample; Normal mean / sample), clip to the env's action space, SeqVectorEnv
 * step with next-step autoreset, and the env's wrapper chain if it has one. Every finished episode is
 * one event (step, env, raw return, length) from the env's RecordEpisodeStatistics state. Returned
 * are the events ordered by (step, env), up to and including every event of the first step at which
 * their count reaches num_eval_runs (the reference's while (size < num_eval_runs) around a loop over
 * all infos of a step): *n_out may exceed num_eval_runs by up to num_eval_envs - 1, and
 * *env_steps_out is that step + 1. PPO_SAMPLE draws with the key (seed, rank, env, step0 + k) at
 * evaluation step k, i.e. ppo_get_action_and_value(env_base = 0, step_id = step0 + k).
 *
 * The work runs on the context stream in chunks of chunk_steps env steps (0: 4096; 512 for
 * PSYN_CARTPOLE), one host synchronisation per chunk; the chunk size changes no returned bit. The
 * event buffer of a chunk holds every event the chunk can produce: an env finishes at most one episode
 * per max_steps + 1 steps, and a PSYN_CARTPOLE env, whose episodes terminate, at most one per 2 steps
 * (num_eval_envs * (chunk_steps / 2 + 2) events of 16 bytes: the reason for its shorter default). For the AC agent (LayerNorm-Beta,
 * hidden 256, obs_dim <= 32, act_dim <= 8) on an env without wrappers a chunk is one persistent launch
 * (k_eval: actor weights resident in registers, the env step fused in); otherwise, and with mode = 1,
 * it is chunk_steps x {act launch, psyn_step, event recorder}. Both give bitwise the same result.
 * ppo_eval_info reports the path the last call took ("eval=k_eval" | "eval=per_step" | "eval=none").
 *
 * Refused (-1, ppo_last_error) before any launch: NULL arguments, num_eval_runs <= 0, num_eval_envs
 * outside [1, E], cap < num_eval_runs + num_eval_envs - 1, PPO_GIVEN, PPO_ROACH on a tanh-Normal
 * agent, env obs / act dims that differ from the agent's. The call does not touch the rollout storage,
 * the iteration counter or the parameters; it leaves the env mid-episode (and its finished-episode
 * sums of psyn_episode_stats include the evaluation's episodes). */
typedef struct ppo_eval_config {
  int  sample_type;     /* PPO_SAMPLE | PPO_MEAN | PPO_ROACH */
  int  eval_seed;
  int  num_eval_envs;   /* 1: ac:965-1001 (env 0 only); E: ppo:589-626 (all envs) */
  int  num_eval_runs;
  long step0;           /* Philox step id of evaluation step 0 (PPO_SAMPLE only) */
  int  chunk_steps;     /* 0 = default (4096; PSYN_CARTPOLE 512); env steps per launch / per read-out */
  int  mode;            /* 0 auto, 1 force the per-step path (tests, A/B) */
} ppo_eval_config;

int ppo_evaluate_synth(struct ppo_ctx* ctx, psyn_t* env, const ppo_eval_config* cfg,
                       float* returns_host, int* lengths_host, int cap, int* n_out, long* env_steps_out);
int ppo_eval_info(const struct ppo_ctx* ctx, char* buf, int len);

#ifdef __cplusplus
}
#endif
#endif
