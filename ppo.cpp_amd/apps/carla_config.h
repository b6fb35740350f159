// apps/carla_config.h — the CaRL trainer's configuration: every option of the reference's GlobalConfig
// (include/carla/carla_config.h) with its name, type and default, described ONCE as a table of fields in
// the order of the reference's to_json. The command-line flags, the JSON sent to the leaderboard gyms and
// written to config.json, and the reader of an earlier run's config.json are loops over that table.
//
// JSON: the reference's keys in its order, "py/object" first (the Python side rebuilds its GlobalConfig
// from it); gpu_ids and ports stay out. Each value has the reference's JSON type; a real is written with
// 17 significant digits, so it parses to exactly (double)(float)field, which is what json_spirit writes
// for the reference's fp32 fields.
//
// Options the trainer itself reads are the ones ac_ppo_carla.cpp uses; everything else (rewards,
// rendering, termination, ...) is stored and forwarded to the gyms, which is all the reference's trainer
// does with them. ttc_resolution, ttc_penalty_ticks and survival_reward_magnitude have no flag there
// either. rdzv_file and collect_mode are this trainer's own flags and are not part of the JSON.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "json_flat.h"
#include "trainer_common.h"

namespace app {

struct GlobalConfig {
  int seed = 1;
  int total_timesteps = 1'000'000;
  float learning_rate = 3e-4f;
  int num_envs = 1;
  int num_steps = 2048;
  float gamma = 0.99f;
  float gae_lambda = 0.95f;
  int num_minibatches = 32;
  int update_epochs = 10;
  bool norm_adv = true;
  float clip_coef = 0.2f;
  bool clip_vloss = true;
  float ent_coef = 0.0f;
  float vf_coef = 0.5f;
  float max_grad_norm = 0.5f;
  float adam_eps = 1e-5f;
  std::string lr_schedule = "linear";
  int num_eval_runs = 10;
  bool clip_actions = true;
  bool torch_deterministic = true;
  std::vector<int> gpu_ids = {0};
  std::string collect_device = "gpu";
  std::string train_device = "gpu";
  std::string rdzv_addr = "localhost";
  int tcp_store_port = 29500;
  int use_dd_ppo_preempt = 0;
  float dd_ppo_min_perc = 0.25f;
  float dd_ppo_preempt_threshold = 0.6f;
  std::vector<int> ports = {5555};
  bool use_exploration_suggest = false;
  bool use_speed_limit_as_max_speed = false;
  float beta_min_a_b_value = 1.0f;
  bool use_new_bev_obs = false;
  int obs_num_channels = 15;
  std::string map_folder = "maps_low_res";
  float pixels_per_meter = 5.0f;
  int route_width = 16;
  std::string reward_type = "roach";
  bool consider_tl = true;
  float eval_time = 1200.0f;
  float terminal_reward = 0.0f;
  bool normalize_rewards = false;
  bool speeding_infraction = false;
  float min_thresh_lat_dist = 3.5f;
  int num_route_points_rendered = 80;
  bool use_green_wave = false;
  std::string image_encoder = "roach";
  bool use_comfort_infraction = false;
  float comfort_penalty_factor = 0.5f;
  bool use_layer_norm = false;
  bool use_vehicle_close_penalty = false;
  bool render_green_tl = true;
  std::string distribution = "beta";
  float weight_decay = 0.0f;
  bool use_termination_hint = false;
  bool use_perc_progress = false;
  float lane_distance_violation_threshold = 0.0f;
  float lane_dist_penalty_softener = 1.0f;
  bool use_min_speed_infraction = false;
  bool use_leave_route_done = true;
  int obs_num_measurements = 8;
  bool use_extra_control_inputs = false;
  bool condition_outside_junction = true;
  bool use_layer_norm_policy_head = true;
  bool use_outside_route_lanes = false;
  bool use_max_change_penalty = false;
  float terminal_hint = 10.0f;
  bool penalize_yellow_light = true;
  bool use_target_point = false;
  float speeding_multiplier = 0.0f;
  bool use_value_measurements = true;
  int bev_semantics_width = 192, bev_semantics_height = 192;
  int num_value_measurements = 3;
  int pixels_ev_to_bottom = 40;
  bool use_history = false;
  std::string team_code_folder = "";
  std::string load_file = "None";
  bool debug = false;
  std::string debug_type = "render";
  std::string logdir = "";
  // counters kept in config.json across restarts
  long global_step = 0;
  float max_training_score = std::numeric_limits<float>::lowest();
  long best_iteration = 0;
  long latest_iteration = 0;
  bool use_off_road_term = false;
  float off_road_term_perc = 0.5f;
  float beta_1 = 0.9f;
  float beta_2 = 0.999f;
  bool render_speed_lines = false;
  bool use_new_stop_sign_detector = false;
  bool use_positional_encoding = false;
  bool use_ttc = false;
  int ttc_resolution = 2;
  int ttc_penalty_ticks = 100;
  bool render_yellow_time = false;
  bool use_single_reward = true;
  bool use_rl_termination_hint = false;
  bool render_shoulder = true;
  bool use_shoulder_channel = true;
  bool use_survival_reward = false;
  float survival_reward_magnitude = 0.0001f;
  // derived from the others (derive)
  int num_devices = 1;
  std::string exp_name = "";
  int batch_size = 0, minibatch_size = 0, num_iterations = 0, num_envs_per_proc = 0;
  int batch_size_per_device = 0, minibatch_per_device = 0;
  // this trainer's own (not in the JSON)
  std::string rdzv_file = "";
  std::string collect_mode = "lockstep";

  void derive(int world_size) {
    num_devices = world_size;
    if (exp_name.empty()) exp_name = "PPO_002_" + std::to_string(seed);
    batch_size = num_steps * num_envs;
    minibatch_size = batch_size / std::max(1, num_minibatches);
    num_iterations = batch_size > 0 ? total_timesteps / batch_size : 0;
    num_envs_per_proc = num_envs / num_devices;
    batch_size_per_device = batch_size / num_devices;
    minibatch_per_device = minibatch_size / num_devices;
  }

  // One JSON key: where it lives, its JSON type and, for keys that are also flags, the help text.
  enum Kind { BOOL, INT, LONG, REAL, STR };
  struct Field {
    const char* name;
    Kind kind;
    void* p;
    const char* help;  // nullptr: no command-line flag
  };

  // the keys after "py/object", in the order of the reference's to_json
  std::vector<Field> fields() {
    auto B = [](const char* n, bool* p, const char* h) { return Field{n, BOOL, p, h}; };
    auto I = [](const char* n, int* p, const char* h) { return Field{n, INT, p, h}; };
    auto L = [](const char* n, long* p, const char* h) { return Field{n, LONG, p, h}; };
    auto R = [](const char* n, float* p, const char* h) { return Field{n, REAL, p, h}; };
    auto S = [](const char* n, std::string* p, const char* h) { return Field{n, STR, p, h}; };
    return {
        I("seed", &seed, "Seed of parameter initialisation, sampling and minibatch order"),
        I("total_timesteps", &total_timesteps, "Environment steps to train for, over all envs"),
        R("learning_rate", &learning_rate, "Initial Adam step size"),
        I("num_envs", &num_envs, "Environments over all ranks; one port each"),
        I("num_steps", &num_steps, "Steps each env collects per iteration"),
        R("gamma", &gamma, "Reward discount"),
        R("gae_lambda", &gae_lambda, "GAE trace decay"),
        I("num_minibatches", &num_minibatches, "Optimizer steps per epoch"),
        I("update_epochs", &update_epochs, "Passes over a collection per iteration"),
        B("norm_adv", &norm_adv, "1: standardise the advantages of each minibatch"),
        R("clip_coef", &clip_coef, "Clipping range of the probability ratio (and of the value change)"),
        B("clip_vloss", &clip_vloss, "1: clipped value loss"),
        R("ent_coef", &ent_coef, "Entropy bonus coefficient"),
        R("vf_coef", &vf_coef, "Value loss coefficient"),
        R("max_grad_norm", &max_grad_norm, "Global gradient norm the update is clipped to"),
        R("adam_eps", &adam_eps, "Adam's epsilon"),
        S("lr_schedule", &lr_schedule, "linear: anneal the step size to 0 over the run; anything else: constant"),
        I("num_eval_runs", &num_eval_runs, "Evaluation environments (stored and forwarded; unused by the trainer)"),
        B("clip_actions", &clip_actions, "1: clamp actions to the env's range before stepping"),
        B("torch_deterministic", &torch_deterministic,
          "Stored and forwarded; this build's kernels are deterministic either way"),
        S("collect_device", &collect_device, "Where collection runs: gpu (cpu is not built)"),
        S("train_device", &train_device, "Where training runs: gpu (cpu is not built)"),
        S("rdzv_addr", &rdzv_addr, "Host of rank 0, for the DD-PPO store"),
        I("tcp_store_port", &tcp_store_port, "Port of the DD-PPO store"),
        I("use_dd_ppo_preempt", &use_dd_ppo_preempt, "1: stragglers stop collecting early (DD-PPO preemption)"),
        R("dd_ppo_min_perc", &dd_ppo_min_perc, "Share of num_steps an env must collect before it may be preempted"),
        R("dd_ppo_preempt_threshold", &dd_ppo_preempt_threshold, "Share of finished envs that triggers preemption"),
        I("num_devices", &num_devices, nullptr),
        S("exp_name", &exp_name, "Experiment folder name under logdir (default PPO_002_<seed>)"),
        I("batch_size", &batch_size, nullptr),
        I("minibatch_size", &minibatch_size, nullptr),
        I("num_iterations", &num_iterations, nullptr),
        I("num_envs_per_proc", &num_envs_per_proc, nullptr),
        I("batch_size_per_device", &batch_size_per_device, nullptr),
        I("minibatch_per_device", &minibatch_per_device, nullptr),
        B("use_exploration_suggest", &use_exploration_suggest, "gym: exploration loss hints (not implemented there)"),
        B("use_speed_limit_as_max_speed", &use_speed_limit_as_max_speed,
          "gym: the ego's current speed limit replaces the reward's maximum speed"),
        R("beta_min_a_b_value", &beta_min_a_b_value, "Added to softplus for the Beta distribution's a and b"),
        B("use_new_bev_obs", &use_new_bev_obs, "gym: render with the newer BEV observation module"),
        I("obs_num_channels", &obs_num_channels, "Channels of the BEV image"),
        S("map_folder", &map_folder, "gym: folder of the preprocessed maps"),
        R("pixels_per_meter", &pixels_per_meter, "gym: BEV resolution"),
        I("route_width", &route_width, "gym: pixels the route is drawn wide"),
        S("reward_type", &reward_type, "gym: reward function, roach or simple_reward"),
        B("consider_tl", &consider_tl, "gym: 0 switches traffic-light infractions off (simple_reward)"),
        R("eval_time", &eval_time, "gym: seconds until an episode is truncated"),
        R("terminal_reward", &terminal_reward, "gym: reward added when an episode ends"),
        B("normalize_rewards", &normalize_rewards, "Stored and forwarded only (reward normalisation is not implemented)"),
        B("speeding_infraction", &speeding_infraction, "gym: driving too fast ends the route"),
        R("min_thresh_lat_dist", &min_thresh_lat_dist, "gym: lateral metres from the lane centre that count as deviation"),
        I("num_route_points_rendered", &num_route_points_rendered, "gym: route points drawn into the BEV"),
        B("use_green_wave", &use_green_wave, "gym: some routes get all-green traffic lights"),
        S("image_encoder", &image_encoder, "CNN encoder: roach or roach_ln"),
        B("use_comfort_infraction", &use_comfort_infraction, "gym: soft penalty beyond the comfort limits"),
        R("comfort_penalty_factor", &comfort_penalty_factor, "gym: largest comfort penalty"),
        B("use_layer_norm", &use_layer_norm, "1: LayerNorm before every ReLU of the MLPs"),
        B("use_vehicle_close_penalty", &use_vehicle_close_penalty, "gym: penalty for tailgating"),
        B("render_green_tl", &render_green_tl, "gym: draw green traffic lights"),
        S("distribution", &distribution, "Action distribution; only beta exists (stored and forwarded)"),
        R("weight_decay", &weight_decay, "Adam's (coupled L2) weight decay"),
        B("use_termination_hint", &use_termination_hint, "gym: speed-dependent penalty on a crash or a red light"),
        B("use_perc_progress", &use_perc_progress, "gym: scale route progress by the distance to the lane centre"),
        R("lane_distance_violation_threshold", &lane_distance_violation_threshold,
          "gym: metres from the lane centre without a penalty"),
        R("lane_dist_penalty_softener", &lane_dist_penalty_softener, "gym: below 1 weakens the lane distance penalty"),
        B("use_min_speed_infraction", &use_min_speed_infraction, "gym: penalty for driving slower than the traffic"),
        B("use_leave_route_done", &use_leave_route_done, "gym: leaving the planned route ends the episode"),
        I("obs_num_measurements", &obs_num_measurements, "Scalars in the measurement vector"),
        B("use_extra_control_inputs", &use_extra_control_inputs, "gym: extra control history in the measurements"),
        B("condition_outside_junction", &condition_outside_junction, "gym: draw the route outside junctions too"),
        B("use_layer_norm_policy_head", &use_layer_norm_policy_head,
          "With use_layer_norm: 0 leaves the policy head without LayerNorm"),
        B("use_outside_route_lanes", &use_outside_route_lanes, "gym: opposing lanes and sidewalks end the route"),
        B("use_max_change_penalty", &use_max_change_penalty, "gym: soft penalty for abrupt action changes"),
        R("terminal_hint", &terminal_hint, "gym: subtracted from the last reward after a collision"),
        B("penalize_yellow_light", &penalize_yellow_light, "gym: running a yellow light counts"),
        B("use_target_point", &use_target_point, "gym: a target point in the measurements"),
        R("speeding_multiplier", &speeding_multiplier, "gym: weight of the speeding penalty"),
        B("use_value_measurements", &use_value_measurements, "gym: 0 zeroes the value head's measurements"),
        I("bev_semantics_width", &bev_semantics_width, "BEV image width in pixels"),
        I("bev_semantics_height", &bev_semantics_height, "BEV image height in pixels"),
        I("num_value_measurements", &num_value_measurements, "Scalars only the value head sees"),
        I("pixels_ev_to_bottom", &pixels_ev_to_bottom, "gym: pixels between the ego vehicle and the image's lower edge"),
        B("use_history", &use_history, "gym: past frames in the BEV observation"),
        S("team_code_folder", &team_code_folder, "Folder of env_agent.py; comm_files/ is created under it (required)"),
        S("load_file", &load_file, "model_latest_<n>.pth to resume from, with its folder's config.json; None: start fresh"),
        B("debug", &debug, "Forwarded to the gyms; the trainer's OpenCV view is not built"),
        S("debug_type", &debug_type, "gym: render or save the debug images"),
        S("logdir", &logdir, "Parent of the experiment folder"),
        L("global_step", &global_step, nullptr),
        R("max_training_score", &max_training_score, nullptr),
        L("best_iteration", &best_iteration, nullptr),
        L("latest_iteration", &latest_iteration, nullptr),
        B("use_off_road_term", &use_off_road_term, "gym: leaving the drivable area ends the episode"),
        R("off_road_term_perc", &off_road_term_perc, "gym: off-road share of the ego's footprint that ends it"),
        R("beta_1", &beta_1, "Adam's first-moment decay"),
        R("beta_2", &beta_2, "Adam's second-moment decay"),
        B("render_speed_lines", &render_speed_lines, "gym: speed lines on moving objects"),
        B("use_new_stop_sign_detector", &use_new_stop_sign_detector, "gym: stop-sign check that lane changes cannot dodge"),
        B("use_positional_encoding", &use_positional_encoding, "1: two coordinate channels (linspace(-1, 1) by row and by column) beside the bev, which is then not divided by 255"),
        B("use_ttc", &use_ttc, "gym: time-to-collision term in the reward"),
        I("ttc_resolution", &ttc_resolution, nullptr),
        I("ttc_penalty_ticks", &ttc_penalty_ticks, nullptr),
        B("render_yellow_time", &render_yellow_time, "gym: encode a yellow light's remaining time"),
        B("use_single_reward", &use_single_reward, "gym: simple_reward from route completion alone"),
        B("use_rl_termination_hint", &use_rl_termination_hint, "gym: red lights count for the termination hint"),
        B("render_shoulder", &render_shoulder, "gym: draw shoulder lanes as road"),
        B("use_shoulder_channel", &use_shoulder_channel, "gym: a channel of their own for shoulder lanes"),
        B("use_survival_reward", &use_survival_reward, "gym: a constant reward every frame"),
        R("survival_reward_magnitude", &survival_reward_magnitude, nullptr),
    };
  }

  // ports_given / gpu_ids_given: value lists replace the default once a value is given
  void add_flags(Flags& flags, std::vector<int>* ports_given, std::vector<int>* gpu_ids_given) {
    for (const Field& f : fields()) {
      if (!f.help) continue;
      switch (f.kind) {
        case BOOL: flags.add(f.name, f.help, static_cast<bool*>(f.p)); break;
        case INT: flags.add(f.name, f.help, static_cast<int*>(f.p)); break;
        case REAL: flags.add(f.name, f.help, static_cast<float*>(f.p)); break;
        case STR: flags.add(f.name, f.help, static_cast<std::string*>(f.p)); break;
        case LONG: break;  // the counters have no flag
      }
    }
    flags.add_list("gpu_ids", "Device of each local rank: --gpu_ids 0 --gpu_ids 1 ...", gpu_ids_given);
    flags.add_list("ports", "Port of each env's leaderboard gym: --ports 5555 --ports 5556 ...", ports_given);
    flags.add("rdzv_file", "File through which rank 0 hands the RCCL id to the other ranks", &rdzv_file);
    flags.add("collect_mode",
              "lockstep: one batched forward per step, envs stepped one after the other; threads: one thread and one "
              "batch-1 forward per env",
              &collect_mode);
  }

  static std::string real_text(float v) {
    char buf[40];
    std::snprintf(buf, sizeof buf, "%.17g", (double)v);
    if (!std::strpbrk(buf, ".enN")) std::strcat(buf, ".0");  // a real stays a real for a typed reader
    return buf;
  }
  static std::string string_text(const std::string& s) {
    std::string o = "\"";
    for (const char c : s) {
      if (c == '"' || c == '\\') o += '\\';
      if (c == '\n') { o += "\\n"; continue; }
      o += c;
    }
    return o + "\"";
  }

  // the object the leaderboard gyms, config.json, a later --load_file and ppo_carla_inference read
  std::string to_json() {
    std::string o = "{\n    \"py/object\" : \"rl_config.GlobalConfig\"";
    for (const Field& f : fields()) {
      o += ",\n    \"" + std::string(f.name) + "\" : ";
      switch (f.kind) {
        case BOOL: o += *static_cast<bool*>(f.p) ? "true" : "false"; break;
        case INT: o += std::to_string(*static_cast<int*>(f.p)); break;
        case LONG: o += std::to_string(*static_cast<long*>(f.p)); break;
        case REAL: o += real_text(*static_cast<float*>(f.p)); break;
        case STR: o += string_text(*static_cast<std::string*>(f.p)); break;
      }
    }
    return o + "\n}\n";
  }

  // every key of an earlier run's config.json that is there (update_from_json); a file of an older
  // trainer with fewer keys leaves the rest at their values
  void update_from_json(const FlatJson& j) {
    for (const Field& f : fields()) {
      if (!j.has(f.name)) continue;
      const std::string& raw = j.raw(f.name);
      switch (f.kind) {
        case BOOL: *static_cast<bool*>(f.p) = j.get_bool(f.name, false); break;
        case INT: *static_cast<int*>(f.p) = (int)std::strtod(raw.c_str(), nullptr); break;
        case LONG: *static_cast<long*>(f.p) = raw.find_first_of(".eE") == std::string::npos
                                                  ? std::strtol(raw.c_str(), nullptr, 10)
                                                  : (long)std::strtod(raw.c_str(), nullptr); break;
        case REAL: *static_cast<float*>(f.p) = (float)std::strtod(raw.c_str(), nullptr); break;
        case STR: *static_cast<std::string*>(f.p) = j.get_string(f.name, ""); break;
      }
    }
  }
};

}  // namespace app
