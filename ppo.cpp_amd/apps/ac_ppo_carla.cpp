// apps/ac_ppo_carla.cpp — drop-in of the training loop of src/carla/ac_ppo_carla.cpp (:284-710): the CaRL
// CNN agent trained with PPO against CARLA leaderboard gyms, one env per port (gymcpp/carla_gym.h).
//
// Per iteration: linear LR anneal (:348-353); collection of num_steps steps over all envs of the
// process (:355-417), in one of two forms (--collect_mode): "lockstep" (default) — one batched
// ppo_carla_rollout_act per step, then one env step per env, one after the other — or "threads" — the
// reference's structure: one std::thread and one act lane (ppo_carla_lane_t: a stream and a private set
// of the forward's buffers) per env, each running its env's steps with batch-1 forwards, so the
// simulators tick at the same time; joined before the statistics all-reduce —; GAE and update_epochs x
// num_minibatches optimizer steps on the device (ppo_carla_rollout_gae / _train, include/ppo_carla.h); the reference's log lines ("global_step=...,
// avg_episodic_return=...", "SPS: ..."), TensorBoard scalars, model_latest_%09d.pth /
// optimizer_latest_%09d.pth with the previous pair removed (:664-683), model_best.pth /
// optimizer_best.pth on a new windowed best (:456-474), config.json beside them. --load_file
// <...>/model_latest_%09d.pth resumes at the next iteration with every setting of that folder's config.json,
// the arguments applied again on top (:90-99), and the optimizer with its archive's betas and weight decay
// (:226-255).
//
// DD-PPO preemption (--use_dd_ppo_preempt 1, :268-282, :343-345, :399-413): rank 0 serves the TCP store,
// every env has a client; an env stops collecting once more than dd_ppo_preempt_threshold of all envs
// are done and it is past dd_ppo_min_perc of its steps. The minimum collected step count over the
// process's envs goes to GAE and train (:422-436).
//
// Ranks: RANK / WORLD_SIZE / LOCAL_RANK (torchrun) or OMPI_COMM_WORLD_* (mpirun); num_envs is the
// total over ranks, each rank connects to ports[num_envs_per_proc * local_rank + i]. The RCCL id
// travels through --rdzv_file. The agent's update averages advantage statistics and gradients.
//
// Flags and config: every option of carla_config.h with its name, type and default (apps/carla_config.h: one
// table for the flags, the JSON sent to the gyms on <port>.conf_lock, config.json and its reader). The
// reward / rendering / termination options are stored and forwarded, as in the reference's trainer; beta_1,
// beta_2 and weight_decay reach the device optimizer (ppo_carla_set_adam) and the optimizer archive. Not
// built: collect_device / train_device cpu, the OpenCV view of --debug 1, roach_ln2. use_positional_encoding
// creates the agent through ppo_carla_create3 (cnn.0 with obs_num_channels + 2 input channels on the
// un-normalised bev, include/ppo_carla.h); checkpoints, config.json and the gyms' JSON carry the switch.
#include <hip/hip_runtime.h>

#include <deque>
#include <iomanip>
#include <map>
#include <numeric>
#include <regex>
#include <set>

#include "../../include/ppo_carla.h"
#include "../../include/ppo_hip.h"
#include "../../include/ppo_pth.h"
#include "../gymcpp/carla_gym.h"
#include "../net/zmtp.h"
#include "carla_config.h"
#include "json_flat.h"
#include "tcp_store.h"
#include "trainer_common.h"

using namespace app;
namespace fs = std::filesystem;

static int env_int(const char* a, const char* b, int def) {
  if (const char* v = std::getenv(a)) return std::atoi(v);
  if (const char* v = std::getenv(b)) return std::atoi(v);
  return def;
}

// Fresh parameters. Linear: LibTorch's default, weight and bias U(+-1 / sqrt(fan_in))
// (kaiming_uniform_(a = sqrt(5))), as the reference's Agent keeps it; LayerNorm weight 1 / bias 0;
// action_space_high / _low from the env. Conv2d: the reference wraps every convolution in _weights_init
// (carla_model.h:45-76, :555-560): xavier_uniform_ with gain sqrt(2), U(+-sqrt(2) * sqrt(6 / (fan_in + fan_out))),
// fan_in = IC * K * K, fan_out = OC * K * K, and bias 0.1. A positional agent's convolutions are drawn that
// way, cnn.0 with IC = obs_num_channels + 2 (+-0.139 at 15 channels). The agents without the switch keep what
// this trainer has always drawn for them, the Linear rule with fan_in = IC * K * K for the convolutions too:
// that departs from the reference and is left for a change of its own, since it alters every existing run.
static std::vector<float> init_carla_params(const ppo_carla_layout2& L, int seed, float hi, float lo) {
  std::vector<float> p(L.P, 0.0f);
  std::mt19937 rng((uint32_t)seed);
  const bool reference_conv_init = L.conv_ic[0] != L.C;
  std::map<long, float> xavier;  // conv weight offset -> bound
  for (int i = 0; i < PPO_CARLA_NCONV; ++i) {
    const float kk = (float)(L.conv_k[i] * L.conv_k[i]);
    xavier[L.conv_w[i]] = std::sqrt(2.0f) * std::sqrt(6.0f / ((float)(L.conv_ic[i] + L.conv_oc[i]) * kk));
  }
  std::set<long> ln;
  for (int i = 0; i < PPO_CARLA_NCONV; ++i) ln.insert(L.conv_g[i]);
  for (int i = 0; i < 2; ++i) {
    ln.insert(L.lin_g[i]); ln.insert(L.st_g[i]); ln.insert(L.v_g[i]); ln.insert(L.pi_g[i]);
  }
  p[L.hi] = hi;
  p[L.lo] = lo;
  for (int t = 2; t + 1 < L.ntensors; t += 2) {  // (weight, bias) pairs in named_parameters() order
    const long w = L.t_off[t], nw = L.t_len[t], b = L.t_off[t + 1], nb = L.t_len[t + 1];
    if (ln.count(w)) {
      std::fill(p.begin() + w, p.begin() + w + nw, 1.0f);
      continue;
    }
    if (reference_conv_init && xavier.count(w)) {
      std::uniform_real_distribution<float> u(-xavier[w], xavier[w]);
      for (long i = 0; i < nw; ++i) p[w + i] = u(rng);
      std::fill(p.begin() + b, p.begin() + b + nb, 0.1f);
      continue;
    }
    const float bound = 1.0f / std::sqrt((float)(nw / nb));
    std::uniform_real_distribution<float> u(-bound, bound);
    for (long i = 0; i < nw; ++i) p[w + i] = u(rng);
    for (long i = 0; i < nb; ++i) p[b + i] = u(rng);
  }
  return p;
}

// save_state (:62-73): model, optimizer and config.json
static void save_state(ppo_carla_t* agent, const ppo_carla_layout2& L, const fs::path& folder,
                       const std::string& model_file, const std::string& optimizer_file, double lr,
                       GlobalConfig& config) {
  std::vector<float> p(L.P), m(L.P), v(L.P);
  long step = 0;
  check(ppo_carla_save_params(agent, p.data(), L.P), "ppo_carla_save_params");
  check(ppo_carla_save_adam(agent, m.data(), v.data(), L.P, &step), "ppo_carla_save_adam");
  check(ppo_carla_pth_save2(&L, p.data(), (folder / model_file).string().c_str()), "torch::save of the model");
  double b1 = 0.0, b2 = 0.0, wd = 0.0;  // the agent's: exactly (0.9, 0.999, 0) unless ppo_carla_set_adam was called
  check(ppo_carla_get_adam(agent, &b1, &b2, &wd), "ppo_carla_get_adam");
  check(ppo_carla_pth_save_adam3(&L, m.data(), v.data(), step, lr, config.adam_eps, b1, b2, wd,
                                 (folder / optimizer_file).string().c_str()),
        "torch::save of the optimizer");
  std::ofstream out((folder / "config.json").string());
  out << config.to_json();
}

int main(int argc, const char** argv) {
  std::ios_base::sync_with_stdio(false);
  const auto process_start = fs::file_time_type::clock::now();
  const int rank = env_int("RANK", "OMPI_COMM_WORLD_RANK", 0);
  const int world_size = env_int("WORLD_SIZE", "OMPI_COMM_WORLD_SIZE", 1);
  const int local_rank = env_int("LOCAL_RANK", "OMPI_COMM_WORLD_LOCAL_RANK", rank);

  GlobalConfig config;
  std::vector<int> ports_given, gpu_ids_given;
  // 0: run, 1: help shown, 2: refused
  auto parse_args = [&]() {
    Flags flags;
    ports_given.clear();
    gpu_ids_given.clear();
    config.add_flags(flags, &ports_given, &gpu_ids_given);
    try {
      flags.parse(argc, argv);
      if (config.collect_mode != "lockstep" && config.collect_mode != "threads")
        throw ParseError("Option 'collect_mode' must be lockstep or threads. Chosen option: " + config.collect_mode);
      if (config.team_code_folder.empty()) throw ParseError("Option 'team_code_folder' is required");
    } catch (const HelpRequested&) {
      flags.print_help(std::cout);
      return 1;
    } catch (const ParseError& e) {
      std::cerr << e.what() << std::endl;
      flags.print_help(std::cerr);
      return 2;
    }
    return 0;
  };
  if (const int rc = parse_args()) return rc - 1;

  // an earlier run (:90-99): every key of the folder's config.json, then the arguments again on top.
  // ports, gpu_ids and team_code_folder are not in the file (or empty there) and come from the arguments.
  int start_step = 0;
  if (config.load_file != "None") {
    const fs::path lf(config.load_file);
    try {
      config.update_from_json(FlatJson::parse_file((lf.parent_path() / "config.json").string()));
    } catch (const std::exception& e) {
      std::cerr << "ac_ppo_carla: " << e.what() << std::endl;
      return 1;
    }
    if (const int rc = parse_args()) return rc - 1;
    std::smatch match;
    const std::string name = lf.filename().string();
    if (std::regex_search(name, match, std::regex("(\\d+)(?=\\.pth)"))) {
      start_step = std::stoi(match.str()) + 1;  // the saved step was already completed
      std::cout << "Start training from step: " << start_step << std::endl;
    }
  }
  // args.hxx value lists replace the default once a value is given here (one port per env is required anyway)
  if (!ports_given.empty()) config.ports = ports_given;
  if (!gpu_ids_given.empty()) config.gpu_ids = gpu_ids_given;
  const std::string& collect_mode = config.collect_mode;
  // :175-197. Collection and training both run on the agent's device in this build.
  for (int k = 0; k < 2; ++k) {
    const std::string& dev = k ? config.train_device : config.collect_device;
    if (dev == "gpu") continue;
    if (dev == "cpu") {
      std::cerr << (k ? "train_device" : "collect_device") << " cpu: CPU mode is not built (DESIGN §7); use gpu"
                << std::endl;
      return k ? 3 : 2;
    }
    if (k) std::cerr << "Unsupported train device selected. Options: cpu, gpu. Selected device: " << dev << std::endl;
    else std::cerr << "Unsupported Collect device selected. Options: cpu, gpu. Selected Device: " << dev << std::endl;
    return k ? 3 : 2;
  }
  if (config.debug) std::cerr << "debug 1 is forwarded to the gyms; the trainer's OpenCV view is not built" << std::endl;
  config.derive(world_size);
  if (config.num_envs_per_proc <= 0 || config.num_envs % world_size != 0) {
    std::cerr << "num_envs must be a positive multiple of the number of ranks\n";
    return 1;
  }
  const int E = config.num_envs_per_proc, T = config.num_steps;
  if ((size_t)(E * (local_rank + 1)) > config.ports.size()) {
    std::cerr << "every env needs a port: pass --ports once per env (" << config.ports.size() << " given, local rank "
              << local_rank << " needs " << E * (local_rank + 1) << ")\n";
    return 1;
  }
  if (config.image_encoder != "roach" && config.image_encoder != "roach_ln") {
    std::cerr << "Unsupported image_encoder chosen. Options roach, roach_ln. Chosen option: " << config.image_encoder
              << std::endl;
    return 1;
  }
  if ((size_t)local_rank >= config.gpu_ids.size()) {
    std::cerr << "local rank " << local_rank << " has no entry in --gpu_ids (" << config.gpu_ids.size()
              << " given): pass one --gpu_ids per local rank\n";
    return 1;
  }
  const std::string config_json = config.to_json();

  try {
    // the config goes to every leaderboard gym of this rank before its env socket exists (:105-126)
    const fs::path comm_folder = fs::path(config.team_code_folder) / "comm_files";
    fs::create_directories(comm_folder);
    for (int i = 0; i < E; ++i) {
      zmtp::Socket socket(zmtp::Type::PAIR);
      const std::string file = std::to_string(config.ports[E * local_rank + i]) + ".conf_lock";
      socket.bind("ipc://" + (comm_folder / file).string());
      socket.send(config_json);
      std::cout << "Connecting to leaderboard gym, port: " << file << std::endl;
      zmtp::Message answer;
      if (!socket.recv(answer)) throw std::runtime_error("Sending config failed.");
      socket.close();
    }
    std::cout << "world_size: " << world_size << "\nrank: " << rank << "\nlocal_rank: " << local_rank << std::endl;

    const fs::path exp_folder = fs::path(config.logdir) / config.exp_name;
    std::unique_ptr<TensorBoardLogger> logger;
    if (rank == 0) {
      fs::create_directories(exp_folder);
      std::ofstream(exp_folder / "config.json") << config_json;
      const auto now_id =
          std::chrono::duration_cast<std::chrono::seconds>(std::chrono::system_clock::now().time_since_epoch()).count();
      logger = std::make_unique<TensorBoardLogger>((exp_folder / ("events.out.tfevents." + std::to_string(now_id) + ".pb")).string());
    }

    // DD-PPO store (:268-282): served by rank 0 from before the communicator exists
    std::unique_ptr<TCPStoreServer> store_server;
    if (config.use_dd_ppo_preempt && rank == 0) {
      store_server = std::make_unique<TCPStoreServer>(config.rdzv_addr, config.tcp_store_port, config.num_envs);
      store_server->start();
    }

    const int device = config.gpu_ids.at((size_t)local_rank);
    HIPCHECK(hipSetDevice(device));

    // envs (:212-220): one SeqVectorEnvCarla of one env per port (clip_actions, next-step autoreset)
    gymcpp::CarlaObsConfig oc{config.obs_num_channels, config.bev_semantics_height, config.bev_semantics_width,
                              config.obs_num_measurements, config.num_value_measurements};
    std::vector<std::shared_ptr<gymcpp::SeqVectorEnvCarla>> envs;
    for (int i = 0; i < E; ++i) {
      auto env_0 = std::make_shared<gymcpp::CarlaEnv>(oc, config.team_code_folder, config.ports[E * local_rank + i]);
      envs.push_back(std::make_shared<gymcpp::SeqVectorEnvCarla>(
          std::vector<std::shared_ptr<gymcpp::EnvironmentWrapperCarla>>{gymcpp::make_env(env_0)}, config.clip_actions));
    }
    const int A = envs[0]->get_action_space(), NM = oc.obs_num_measurements, NV = oc.num_value_measurements;
    const size_t nb = (size_t)oc.obs_num_channels * oc.bev_semantics_height * oc.bev_semantics_width;

    // agent (:222-255)
    ppo_carla_arch arch{config.image_encoder == "roach_ln" ? 1 : 0, config.use_layer_norm ? 1 : 0,
                        config.use_layer_norm_policy_head ? 1 : 0};
    ppo_carla_config cc;
    std::memset(&cc, 0, sizeof(cc));
    cc.obs_channels = oc.obs_num_channels;
    cc.bev_h = oc.bev_semantics_height;
    cc.bev_w = oc.bev_semantics_width;
    cc.num_measurements = NM;
    cc.num_value_measurements = NV;
    cc.action_dim = A;
    cc.beta_min = config.beta_min_a_b_value;
    cc.max_batch = std::max(E, config.minibatch_per_device);
    cc.seed = (uint64_t)config.seed;
    cc.rank = rank;
    ppo_carla_t* agent = nullptr;
    check(ppo_carla_create3(&cc, &arch, config.use_positional_encoding ? 1 : 0, device, nullptr, &agent),
          "ppo_carla_create3");
    ppo_carla_layout2 L;
    check(ppo_carla_get_layout2(agent, &L), "ppo_carla_get_layout2");
    std::vector<float> p0;
    if (config.load_file != "None") {
      p0.resize(L.P);
      check(ppo_carla_pth_load2(&L, config.load_file.c_str(), p0.data(), L.P), "torch::load of the model");
    } else {
      p0 = init_carla_params(L, config.seed, envs[0]->get_action_space_max(), envs[0]->get_action_space_min());
    }
    check(ppo_carla_load_params(agent, p0.data(), L.P), "ppo_carla_load_params");
    // :246 Adam(lr).eps(adam_eps).weight_decay(weight_decay).betas(beta_1, beta_2), the fp32 fields widened.
    // At the defaults the agent keeps its exact (0.9, 0.999, 0) and the default kernel.
    if (config.beta_1 != 0.9f || config.beta_2 != 0.999f || config.weight_decay != 0.0f)
      check(ppo_carla_set_adam(agent, (double)config.beta_1, (double)config.beta_2, (double)config.weight_decay),
            "ppo_carla_set_adam");
    if (world_size > 1) {  // the RCCL id travels through a file, as in ac_ppo_continuous_action
      const std::string path = config.rdzv_file.empty() ? "/tmp/ppo_carla_rdzv_" + std::to_string(config.tcp_store_port) + ".id"
                                                        : config.rdzv_file;
      char id[PPO_COMM_ID_BYTES];
      if (rank == 0) {
        std::error_code ec;
        fs::remove(path, ec);
        check(ppo_comm_unique_id(id), "ppo_comm_unique_id");
        std::ofstream(path + ".tmp", std::ios::binary | std::ios::trunc).write(id, PPO_COMM_ID_BYTES);
        fs::rename(path + ".tmp", path);
      } else {
        const auto not_before = process_start - std::chrono::seconds(30);
        for (int tries = 0;; ++tries) {
          if (tries > 6000) throw std::runtime_error("timed out waiting for " + path + " (rank 0's communicator id)");
          std::error_code ec;
          if (fs::exists(path, ec) && fs::last_write_time(path, ec) >= not_before && !ec &&
              std::ifstream(path, std::ios::binary).read(id, PPO_COMM_ID_BYTES))
            break;
          std::this_thread::sleep_for(std::chrono::milliseconds(10));
        }
      }
      check(ppo_carla_comm_init(agent, id, rank, world_size), "ppo_carla_comm_init");
      if (rank == 0) {
        std::error_code ec;
        fs::remove(path, ec);
      }
      check(ppo_carla_comm_broadcast_params(agent, 0), "ppo_carla_comm_broadcast_params");  // :241-244
    }
    if (config.load_file != "None") {  // :248-255
      const std::string opt_path = std::regex_replace(config.load_file, std::regex("model_"), "optimizer_");
      std::vector<float> m(L.P), v(L.P);
      long step = 0;
      double b1 = 0.0, b2 = 0.0, wd = 0.0, c1 = 0.0, c2 = 0.0, cwd = 0.0;
      check(ppo_carla_pth_load_adam3(&L, opt_path.c_str(), m.data(), v.data(), L.P, &step, nullptr, nullptr, &b1, &b2,
                                     &wd),
            "torch::load of the optimizer");
      check(ppo_carla_load_adam(agent, m.data(), v.data(), L.P, step), "ppo_carla_load_adam");
      // torch::load(optimizer) assigns the saved options to the optimizer: the archive's betas and weight
      // decay replace the configured ones (the learning rate is set per iteration, eps stays adam_eps)
      check(ppo_carla_get_adam(agent, &c1, &c2, &cwd), "ppo_carla_get_adam");
      if (b1 != c1 || b2 != c2 || wd != cwd) {
        std::cout << "Optimizer options from " << opt_path << " replace the configured ones: betas (" << b1 << ", "
                  << b2 << "), weight_decay " << wd << std::endl;
        check(ppo_carla_set_adam(agent, b1, b2, wd), "ppo_carla_set_adam");
      }
      if (rank == 0) logger->add_scalar("charts/restart", (int)config.global_step, 1.0);
    }
    if (rank == 0) std::cout << "Number of parameters in model: " << (L.P - 2) << std::endl;

    ppo_carla_rollout_config rc;
    std::memset(&rc, 0, sizeof(rc));
    rc.num_steps = T;
    rc.num_envs = E;
    rc.update_epochs = config.update_epochs;
    rc.num_minibatches = config.num_minibatches;
    rc.gamma = config.gamma;
    rc.gae_lambda = config.gae_lambda;
    rc.seed = (uint64_t)config.seed;
    rc.rank = rank;
    ppo_carla_rollout_t* roll = nullptr;
    check(ppo_carla_rollout_create(agent, &rc, &roll), "ppo_carla_rollout_create");
    check(ppo_carla_rollout_set_iteration(roll, start_step), "ppo_carla_rollout_set_iteration");
    std::vector<ppo_carla_lane_t*> lanes;  // --collect_mode threads: one per env
    if (collect_mode == "threads") {
      if (E > PPO_CARLA_MAX_LANES)
        throw std::runtime_error("--collect_mode threads serves at most " + std::to_string(PPO_CARLA_MAX_LANES) +
                                 " envs per process");
      lanes.resize(E, nullptr);
      for (int i = 0; i < E; ++i) check(ppo_carla_lane_create(roll, &lanes[i]), "ppo_carla_lane_create");
    }
    const ppo_carla_train_config tc{config.clip_coef, config.ent_coef, config.vf_coef, config.max_grad_norm,
                                    config.adam_eps, config.norm_adv ? 1 : 0, config.clip_vloss ? 1 : 0};

    std::vector<std::unique_ptr<TCPStoreClient>> tcp_clients;
    if (config.use_dd_ppo_preempt)
      for (int i = 0; i < E; ++i)
        tcp_clients.push_back(std::make_unique<TCPStoreClient>(config.rdzv_addr, config.tcp_store_port));

    // next observation of every env, host (pinned) and device
    uint8_t *h_bev = nullptr, *d_bev = nullptr;
    float *h_f = nullptr, *d_f = nullptr;  // meas [E, NM] | vmeas [E, NV] | done [E] | reward [E] | actions [E, A] | sums [3]
    const size_t o_meas = 0, o_vmeas = o_meas + (size_t)E * NM, o_done = o_vmeas + (size_t)E * NV, o_rew = o_done + E,
                 o_act = o_rew + E, o_sum = o_act + (size_t)E * A, nf = o_sum + 3;
    HIPCHECK(hipHostMalloc((void**)&h_bev, nb * E));
    HIPCHECK(hipHostMalloc((void**)&h_f, sizeof(float) * nf));
    HIPCHECK(hipMalloc((void**)&d_bev, nb * E));
    HIPCHECK(hipMalloc((void**)&d_f, sizeof(float) * nf));
    std::fill(h_f, h_f + nf, 0.0f);
    auto put_obs = [&](int i, const gymcpp::SeqVectorEnvCarla::State& s) {
      std::memcpy(h_bev + nb * i, s.bev_semantics, nb);
      std::memcpy(h_f + o_meas + (size_t)NM * i, s.measurements, sizeof(float) * NM);
      std::memcpy(h_f + o_vmeas + (size_t)NV * i, s.value_measurements, sizeof(float) * NV);
    };
    auto upload = [&](int e0, int e1) {  // the observation rows and dones of envs [e0, e1)
      const size_t n = (size_t)(e1 - e0);
      HIPCHECK(hipMemcpy(d_bev + nb * e0, h_bev + nb * e0, nb * n, hipMemcpyHostToDevice));
      HIPCHECK(hipMemcpy(d_f + o_meas + (size_t)NM * e0, h_f + o_meas + (size_t)NM * e0, sizeof(float) * NM * n,
                         hipMemcpyHostToDevice));
      HIPCHECK(hipMemcpy(d_f + o_vmeas + (size_t)NV * e0, h_f + o_vmeas + (size_t)NV * e0, sizeof(float) * NV * n,
                         hipMemcpyHostToDevice));
      HIPCHECK(hipMemcpy(d_f + o_done + e0, h_f + o_done + e0, sizeof(float) * n, hipMemcpyHostToDevice));
    };
    for (int i = 0; i < E; ++i) put_obs(i, envs[i]->reset(config.seed + i));  // :309-313

    std::deque<float> avg_returns;
    const size_t avg_returns_maxlen = 100;
    const auto start_time = std::chrono::high_resolution_clock::now();
    long local_processed_samples = 0;
    std::vector<int> collected(E);
    std::vector<char> active(E);

    for (int iteration = start_step; iteration < config.num_iterations; ++iteration) {
      if (rank == 0 && config.use_dd_ppo_preempt) tcp_clients[0]->reset();  // :343-345
      h_f[o_sum] = 0.0f;  // :346 comm->allreduce(sychronize): every rank starts after the reset
      HIPCHECK(hipMemcpy(d_f + o_sum, h_f + o_sum, sizeof(float), hipMemcpyHostToDevice));
      check(ppo_carla_comm_allreduce(agent, d_f + o_sum, 1, 0), "ppo_carla_comm_allreduce");

      float lrnow = config.learning_rate;
      if (config.lr_schedule == "linear") {  // :348-353
        const float frac = 1.0f - static_cast<float>(iteration) / static_cast<float>(config.num_iterations);
        lrnow = frac * config.learning_rate;
      }

      float sum_r = 0.0f, sum_l = 0.0f, sum_n = 0.0f;
      std::fill(active.begin(), active.end(), 1);
      std::fill(collected.begin(), collected.end(), T);
      // ---- collection (:355-417), one thread and one lane per env ----
      if (collect_mode == "threads") {
        std::vector<float> t_r(E, 0.0f), t_l(E, 0.0f), t_n(E, 0.0f);
        std::vector<std::string> failed(E);
        std::vector<std::thread> threads;
        for (int i = 0; i < E; ++i)
          threads.emplace_back([&, i] {
            try {
              std::vector<float> action((size_t)A);
              for (int step = 0; step < T; ++step) {
                check(ppo_carla_lane_act(lanes[i], step, i, h_bev + nb * i, h_f + o_meas + (size_t)NM * i,
                                         h_f + o_vmeas + (size_t)NV * i, h_f[o_done + i], action.data()),
                      "ppo_carla_lane_act");
                auto [state, reward, termination, truncation, infos] = envs[i]->step(action.data());  // :381
                put_obs(i, state);
                check(ppo_carla_lane_reward(lanes[i], step, i, reward[0]), "ppo_carla_lane_reward");  // :385
                h_f[o_done + i] = (termination[0] != 0.0f || truncation[0] != 0.0f) ? 1.0f : 0.0f;   // :383
                if ((*infos)[0].has_value()) {
                  t_r[i] += (*infos)[0]->r;
                  t_l[i] += (float)(*infos)[0]->l;
                  t_n[i] += 1.0f;
                }
                if (config.use_dd_ppo_preempt) {  // :399-407, this env's own store client
                  const int num_done = tcp_clients[i]->get();
                  const long min_steps = std::lround(config.dd_ppo_min_perc * static_cast<float>(T));
                  if (static_cast<float>(num_done) / static_cast<float>(config.num_envs) > config.dd_ppo_preempt_threshold &&
                      step > min_steps) {
                    std::cout << "Rank: " + std::to_string(rank) + ", Thread: " + std::to_string(i) +
                                     ", Preempt at step: " + std::to_string(step) +
                                     " Num done: " + std::to_string(num_done) + '\n';
                    active[i] = 0;
                    collected[i] = step;  // this step is stored, not trained on
                    tcp_clients[i]->increment();
                    break;
                  }
                }
              }
              if (config.use_dd_ppo_preempt && active[i]) tcp_clients[i]->increment();  // :410-412
            } catch (const std::exception& e) {
              failed[i] = e.what();
              if (failed[i].empty()) failed[i] = "collection thread failed";
            }
          });
        for (auto& t : threads) t.join();  // before the statistics all-reduce (:417)
        for (int i = 0; i < E; ++i)
          if (!failed[i].empty()) throw std::runtime_error("env " + std::to_string(i) + ": " + failed[i]);
        for (int i = 0; i < E; ++i) {  // in env order: thread timing does not reach the sums
          sum_r += t_r[i];
          sum_l += t_l[i];
          sum_n += t_n[i];
        }
      }
      // ---- collection (:355-417), the envs of this process in lockstep ----
      for (int step = 0; collect_mode == "lockstep" && step < T; ++step) {
        int live = 0;
        for (int e0 = 0; e0 < E;) {  // maximal runs of envs that still collect
          if (!active[e0]) { ++e0; continue; }
          int e1 = e0;
          while (e1 < E && active[e1]) ++e1;
          upload(e0, e1);
          check(ppo_carla_rollout_act(roll, step, e0, e1, d_bev + nb * e0, d_f + o_meas + (size_t)NM * e0,
                                      d_f + o_vmeas + (size_t)NV * e0, d_f + o_done + e0, d_f + o_act + (size_t)A * e0,
                                      nullptr),
                "ppo_carla_rollout_act");
          live += e1 - e0;
          e0 = e1;
        }
        if (!live) break;
        check(ppo_device_sync(), "ppo_device_sync");  // the forward runs on the agent's own stream
        HIPCHECK(hipMemcpy(h_f + o_act, d_f + o_act, sizeof(float) * E * A, hipMemcpyDeviceToHost));
        for (int i = 0; i < E; ++i) {
          if (!active[i]) continue;
          auto [state, reward, termination, truncation, infos] = envs[i]->step(h_f + o_act + (size_t)A * i);  // :381
          put_obs(i, state);
          h_f[o_rew + i] = reward[0];
          h_f[o_done + i] = (termination[0] != 0.0f || truncation[0] != 0.0f) ? 1.0f : 0.0f;  // :383
          if ((*infos)[0].has_value()) {
            sum_r += (*infos)[0]->r;
            sum_l += (float)(*infos)[0]->l;
            sum_n += 1.0f;
          }
          if (config.use_dd_ppo_preempt) {  // :399-407
            const int num_done = tcp_clients[i]->get();
            const long min_steps = std::lround(config.dd_ppo_min_perc * static_cast<float>(T));
            if (static_cast<float>(num_done) / static_cast<float>(config.num_envs) > config.dd_ppo_preempt_threshold &&
                step > min_steps) {
              std::cout << "Rank: " << rank << ", Thread: " << i << ", Preempt at step: " << step
                        << " Num done: " << num_done << '\n';
              active[i] = 0;
              collected[i] = step;  // this step is stored, not trained on
              tcp_clients[i]->increment();
            }
          }
        }
        HIPCHECK(hipMemcpy(d_f + o_rew, h_f + o_rew, sizeof(float) * E, hipMemcpyHostToDevice));
        check(ppo_carla_rollout_reward(roll, step, 0, E, d_f + o_rew, nullptr), "ppo_carla_rollout_reward");
      }
      if (config.use_dd_ppo_preempt && collect_mode == "lockstep")  // :410-412
        for (int i = 0; i < E; ++i)
          if (active[i]) tcp_clients[i]->increment();
      const int num_train_steps_per_env = *std::min_element(collected.begin(), collected.end());  // :422-436
      upload(0, E);

      // episode statistics summed over ranks (:419-441)
      h_f[o_sum] = sum_r; h_f[o_sum + 1] = sum_l; h_f[o_sum + 2] = sum_n;
      HIPCHECK(hipMemcpy(d_f + o_sum, h_f + o_sum, sizeof(float) * 3, hipMemcpyHostToDevice));
      check(ppo_carla_comm_allreduce(agent, d_f + o_sum, 3, 0), "ppo_carla_comm_allreduce");
      HIPCHECK(hipMemcpy(h_f + o_sum, d_f + o_sum, sizeof(float) * 3, hipMemcpyDeviceToHost));
      config.global_step += (long)config.num_envs * T;  // duplicated samples of a preempted collection count (:443-445)
      local_processed_samples += (long)config.num_envs * T;
      if (rank == 0 && h_f[o_sum + 2] > 0.0f) {  // :448-476
        const float avg_return = h_f[o_sum] / h_f[o_sum + 2], avg_length = h_f[o_sum + 1] / h_f[o_sum + 2];
        avg_returns.push_back(avg_return);
        if (avg_returns.size() > avg_returns_maxlen) avg_returns.pop_front();
        const float windowed = std::accumulate(avg_returns.begin(), avg_returns.end(), 0.0f) / (float)avg_returns.size();
        logger->add_scalar("charts/episodic_return", (int)config.global_step, avg_return);
        logger->add_scalar("charts/windowed_avg_return", (int)config.global_step, windowed);
        logger->add_scalar("charts/episodic_length", (int)config.global_step, avg_length);
        std::cout << "global_step=" << config.global_step << ", avg_episodic_return=" << std::fixed
                  << std::setprecision(2) << avg_return << " \n";
        if (windowed > config.max_training_score) {
          config.max_training_score = windowed;
          if (config.best_iteration != iteration) {
            config.best_iteration = iteration;
            save_state(agent, L, exp_folder, "model_best.pth", "optimizer_best.pth", lrnow, config);
          }
        }
      }

      // ---- GAE and the epoch loop (:484-621) ----
      check(ppo_carla_rollout_gae(roll, d_bev, d_f + o_meas, d_f + o_vmeas, d_f + o_done, num_train_steps_per_env, nullptr),
            "ppo_carla_rollout_gae");
      ppo_carla_update_stats st;
      float avg_clipfrac = 0.0f;
      check(ppo_carla_rollout_train(roll, &tc, lrnow, num_train_steps_per_env, nullptr, &st, &avg_clipfrac),
            "ppo_carla_rollout_train");
      config.latest_iteration = iteration;
      float returns_mean = 0.0f;  // :626-658, :701: a collective, so every rank calls it
      check(ppo_carla_rollout_returns_mean(roll, num_train_steps_per_env, &returns_mean), "ppo_carla_rollout_returns_mean");

      if (rank == 0) {  // :661-705
        char mf[64], of[64];
        std::snprintf(mf, sizeof mf, "model_latest_%09d.pth", iteration);
        std::snprintf(of, sizeof of, "optimizer_latest_%09d.pth", iteration);
        save_state(agent, L, exp_folder, mf, of, lrnow, config);
        cleanup_checkpoints(exp_folder, iteration);
        const float secs = std::chrono::duration<float>(std::chrono::high_resolution_clock::now() - start_time).count();
        float sps = 0.0f;
        if (secs > 0) {
          sps = static_cast<float>(local_processed_samples) / secs;
          std::cout << std::fixed << std::setprecision(0) << "SPS: " << sps << std::endl;
        }
        const int gs = (int)config.global_step;
        logger->add_scalar("charts/learning_rate", gs, lrnow);
        logger->add_scalar("losses/value_loss", gs, st.v_loss);
        logger->add_scalar("losses/policy_loss", gs, st.pg_loss);
        logger->add_scalar("losses/entropy", gs, st.entropy);
        logger->add_scalar("losses/old_approx_kl", gs, st.old_approx_kl);
        logger->add_scalar("losses/approx_kl", gs, st.approx_kl);
        logger->add_scalar("losses/clipfrac", gs, avg_clipfrac);
        logger->add_scalar("losses/discounted_returns", gs, returns_mean);
        logger->add_scalar("charts/SPS", gs, sps);
        logger->add_scalar("charts/restart", gs, 0.0);
      }
      std::cout << std::flush;
    }

    for (ppo_carla_lane_t* l : lanes) check(ppo_carla_lane_destroy(l), "ppo_carla_lane_destroy");
    ppo_carla_rollout_destroy(roll);
    ppo_carla_destroy(agent);
    (void)hipHostFree(h_bev);
    (void)hipHostFree(h_f);
    (void)hipFree(d_bev);
    (void)hipFree(d_f);
  } catch (const std::exception& e) {
    std::cerr << "ac_ppo_carla: " << e.what() << std::endl;
    return 6;
  }
  return 0;
}
