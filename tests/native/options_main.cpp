// Stand-alone driver of csrc/options.cpp for a sanitizer build (host code only:
// g++ -fsanitize=address,undefined options.cpp options_main.cpp).  Walks the
// table, then reads "name value answer" lines from stdin (answer: the expected
// read-back, or EINVAL) and runs each through the check and store code that
// mfea_set_option uses.  Exit status 0 and "ok <options> <probes>" when all agree.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "options.hpp"

using namespace mfea;

int main() {
  for (int i = 0; i < option_count(); ++i) {
    const OptionDesc& d = option_at(i);
    const int64_t dflt = option_default(d);
    Options o;
    if (find_option(d.name) != &d || !option_legal(d, dflt)) return std::printf("%s: table\n", d.name), 1;
    option_store(d, o, dflt);
    if (d.load(o) != dflt || !d.legal_text[0]) return std::printf("%s: default\n", d.name), 1;
    (void)option_keeps(d, dflt);
  }
  if (find_option("no_such_option")) return 1;
  char name[64], answer[32];
  int64_t value;
  long probes = 0;
  while (std::scanf("%63s %" SCNd64 " %31s", name, &value, answer) == 3) {
    const OptionDesc* d = find_option(name);
    if (!d) return std::printf("%s: unknown\n", name), 1;
    char got[32] = "EINVAL";
    if (option_legal(*d, value)) {
      Options o;
      option_store(*d, o, value);
      std::snprintf(got, sizeof got, "%" PRId64, d->load(o));
    }
    if (std::strcmp(got, answer) != 0) return std::printf("%s %" PRId64 ": %s, not %s\n", name, value, got, answer), 1;
    ++probes;
  }
  std::printf("ok %d %ld\n", option_count(), probes);
  return 0;
}
