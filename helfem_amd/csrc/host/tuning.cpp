#include "tuning.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace helfem {
/// the only place of the library that reads the environment
static Tuning parse(Tuning t, bool live_only) {
#define X(field, type, def, name, live, kind, value, meaning) \
  if (const char *e = (live || !live_only) ? getenv(name) : nullptr; live || !live_only) t.field = e ? (type)(value) : (type)(def);
  HELFEM_TUNING(X)
#undef X
  return t;
}
const Tuning &tuning() {
  static const Tuning snapshot = parse(Tuning(), false);
  return snapshot;
}
Tuning tuning_live() { return parse(tuning(), true); }
static std::string show(bool v) { return v ? "on" : "off"; }
static std::string show(const std::string &v) { return v; }
static std::string show(TrdMode v) { return v == TrdMode::persistent ? "persistent" : v == TrdMode::chain ? "chain" : v == TrdMode::twokernel ? "twokernel" : "unblocked"; }
static std::string show(RsTei v) { return v == RsTei::dev ? "dev" : "host"; }
static std::string show(EigSel v) { return v == EigSel::stein ? "stein" : v == EigSel::dc ? "dc" : "crossover"; }
template <class T> static std::string show(T v) { return std::to_string(v); }
std::string tuning_table() {
  const Tuning now = tuning_live(), def;
  std::string s;
#define X(field, type, d, name, live, kind, value, meaning) \
  s += std::string(name) + "\t" + kind + "\t" + show(def.field) + "\t" + show(now.field) + "\t" + (live ? "live" : "once") + "\t" + meaning + "\n";
  HELFEM_TUNING(X)
#undef X
  return s;
}
}  // namespace helfem
