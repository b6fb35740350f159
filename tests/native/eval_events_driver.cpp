// Stand-alone check of ppo_evaluate_synth's host-side stopping rule (csrc/ppo_eval_events.hpp,
// eval_select) on made-up event lists; built and run by tests/test_eval_cpu.py under
// -fsanitize=address,undefined. Prints one line per case; exit code 0 when every case holds.
#include <cstdio>
#include <random>

#include "ppo_eval_events.hpp"

static int failures = 0;
#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } \
  } while (0)

static EvalEvent ev(long long step, int env) { return EvalEvent{step, env, 1000, (float)(step * 100 + env), 0}; }

int main() {
  long long stop = -1;
  {  // nothing / too few events: more steps are needed
    std::vector<EvalEvent> e;
    CHECK(eval_select(e, 1, &stop) == 0);
    e = {ev(999, 0)};
    CHECK(eval_select(e, 2, &stop) == 0 && stop == -1);
    CHECK(eval_select(e, 0, &stop) == 0);
  }
  {  // one env, two runs: exactly two, stop at the second
    std::vector<EvalEvent> e = {ev(2000, 0), ev(999, 0), ev(3001, 0)};
    CHECK(eval_select(e, 2, &stop) == 2 && stop == 2000);
    CHECK(e[0].step == 999 && e[1].step == 2000);
  }
  {  // three envs finishing together, 4 runs: all 6 of the first two finishing steps, env order in a step
    std::vector<EvalEvent> e = {ev(2000, 2), ev(999, 1), ev(2000, 0), ev(999, 2), ev(3001, 1), ev(999, 0), ev(2000, 1)};
    CHECK(eval_select(e, 4, &stop) == 6 && stop == 2000);
    for (int i = 0; i < 6; ++i) CHECK(e[i].step == (i < 3 ? 999 : 2000) && e[i].env == i % 3);
    CHECK(eval_select(e, 3, &stop) == 3 && stop == 999);
    CHECK(eval_select(e, 7, &stop) == 7 && stop == 3001);
    CHECK(eval_select(e, 8, &stop) == 0);
  }
  {  // shuffled lists: the result does not depend on the arrival order
    std::mt19937 rng(5);
    std::vector<EvalEvent> base;
    for (int env = 0; env < 37; ++env)
      for (int k = 0; k < 4; ++k) base.push_back(ev(999 + 1001LL * k + (env % 5), env));
    std::vector<EvalEvent> ref = base;
    const size_t n0 = eval_select(ref, 50, &stop);
    const long long stop0 = stop;
    CHECK(n0 >= 50 && n0 <= 50 + 36);
    for (int rep = 0; rep < 20; ++rep) {
      std::vector<EvalEvent> s = base;
      std::shuffle(s.begin(), s.end(), rng);
      CHECK(eval_select(s, 50, &stop) == n0 && stop == stop0);
      for (size_t i = 0; i < n0; ++i) CHECK(s[i].step == ref[i].step && s[i].env == ref[i].env && s[i].ret == ref[i].ret);
      for (size_t i = 1; i < s.size(); ++i)
        CHECK(s[i - 1].step < s[i].step || (s[i - 1].step == s[i].step && s[i - 1].env < s[i].env));
    }
  }
  std::printf("%s\n", failures ? "eval_select: FAILED" : "eval_select: ok");
  return failures ? 1 : 0;
}
