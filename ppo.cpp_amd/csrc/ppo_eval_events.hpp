// ppo_eval_events.hpp — episode events of ppo_evaluate_synth and its stopping rule. Plain C++ (no
// HIP): the device kernels write EvalEvent records in any order; the host orders and cuts them here.
#pragma once

#include <algorithm>
#include <vector>

struct EvalEvent {
  long long step;  // evaluation step (0-based) whose env step finished the episode
  int env;
  int len;         // RecordEpisodeStatistics episode length
  float ret;       // ... and raw episodic return
  int pad_;
};

// The reference's `while (episodic_returns.size() < num_eval_runs)` around a loop over all infos of a
// step (ac:965-1001, ppo:589-626): orders ev by (step, env) and returns how many leading events are
// kept: all events of every step up to and including the first step at which the count reaches
// num_runs. 0 when ev holds fewer than num_runs events (more steps are needed). *stop_step is the
// step of the last kept event.
inline size_t eval_select(std::vector<EvalEvent>& ev, int num_runs, long long* stop_step) {
  std::sort(ev.begin(), ev.end(), [](const EvalEvent& a, const EvalEvent& b) {
    return a.step != b.step ? a.step < b.step : a.env < b.env;
  });
  if (num_runs <= 0 || ev.size() < (size_t)num_runs) return 0;
  const long long stop = ev[(size_t)num_runs - 1].step;
  size_t n = (size_t)num_runs;
  while (n < ev.size() && ev[n].step == stop) ++n;
  if (stop_step) *stop_step = stop;
  return n;
}
