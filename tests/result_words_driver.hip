// Host-side driver of tests/test_result_words_host.py: the result-word protocol of csrc/grid_sync.hpp (publish_words,
// words_checksum, words_ready) exercised on ordinary memory, no GPU.
//   driver pairs                the (cap, k) pairs of the library's three pinned buffers, from the header's constants
//   driver check CAP K SEQ      every property below for launches SEQ and SEQ + 1; one "PASS name" / "FAIL name" line each
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"
#include "grid_sync.hpp"

namespace {

typedef unsigned long long u64;

int failures = 0;
void report(const std::string &name, bool ok) {
  printf("%s %s\n", ok ? "PASS" : "FAIL", name.c_str());
  if (!ok) ++failures;
}

// word q of launch seq: NaN, -0.0 and all-ones among them; differs from launch seq - 1's word q for every q
u64 payload(u64 seq, int q) {
  const u64 special[3] = {word_bits(std::nan("")), word_bits(-0.0), ~0ull};
  if ((q + (int)(seq % 2)) % 4 == 0) return special[(q / 4 + seq) % 3];
  u64 v = (seq + 1) * 0x9E3779B97F4A7C15ull + (u64)(q + 1) * 0xBF58476D1CE4E5B9ull;
  v ^= v >> 29;
  return v;
}

void publish(std::vector<double> &buf, int cap, int k, u64 seq) {
  volatile double *host = buf.data();
  publish_words(host, cap, k, seq, [&](int q) { return __builtin_bit_cast(double, payload(seq, q)); });
}

bool ready(const std::vector<double> &buf, int cap, int k, u64 seq, std::vector<u64> *got = nullptr) {
  std::vector<double> out((size_t)cap + 2, 0.0);
  const bool ok = words_ready(reinterpret_cast<const volatile u64 *>(buf.data()), cap, k, seq, out.data());
  if (ok && got) {
    got->resize((size_t)k);
    memcpy(got->data(), out.data(), sizeof(u64) * (size_t)k);
  }
  return ok;
}

void check(int cap, int k, u64 seq) {
  const std::string tag = "seq" + std::to_string(seq) + " ";
  // the buffer as launch seq - 1 left it (seq - 1 == 0: as allocated), then launch seq's words
  std::vector<double> prev((size_t)cap + 2, 0.0);
  if (seq > 1) publish(prev, cap, k, seq - 1);
  std::vector<double> cur = prev;
  publish(cur, cap, k, seq);

  bool differ = true, specials[3] = {false, false, false};
  for (int q = 0; q < k; ++q) {
    differ = differ && payload(seq, q) != payload(seq - 1, q);
    specials[0] |= std::isnan(__builtin_bit_cast(double, payload(seq, q))) && payload(seq, q) != ~0ull;
    specials[1] |= payload(seq, q) == word_bits(-0.0);
    specials[2] |= payload(seq, q) == ~0ull;
  }
  report(tag + "payloads_differ_from_previous_launch", differ);
  if (k >= 13) report(tag + "payloads_hold_nan_negzero_allones", specials[0] && specials[1] && specials[2]);

  std::vector<u64> got;
  bool same = ready(cur, cap, k, seq, &got);
  for (int q = 0; same && q < k; ++q) same = got[(size_t)q] == payload(seq, q);
  report(tag + "published_accepted_bitwise", same);
  report(tag + "previous_launch_refused_for_seq", !ready(prev, cap, k, seq));
  report(tag + "published_refused_for_other_seq", !ready(cur, cap, k, seq - 1) && !ready(cur, cap, k, seq + 1));

  const std::vector<double> zero((size_t)cap + 2, 0.0);
  bool zero_refused = true;
  for (u64 s = 0; s < 4096; ++s) zero_refused = zero_refused && !ready(zero, cap, k, s);
  for (u64 s : {seq - 1, seq, seq + 1, ~0ull, 1ull << 63, (u64)k << 56, WORDS_CHECK_SALT, WORDS_CHECK_SALT ^ ((u64)k << 56)})
    zero_refused = zero_refused && !ready(zero, cap, k, s);
  report(tag + "zero_buffer_refused", zero_refused);

  bool stale_refused = true;
  for (int q = 0; q < k; ++q) {
    std::vector<double> torn = cur;
    torn[(size_t)q] = __builtin_bit_cast(double, payload(seq - 1, q));
    stale_refused = stale_refused && !ready(torn, cap, k, seq);
  }
  report(tag + "stale_value_word_refused", stale_refused);
  {
    std::vector<double> torn = cur;
    torn[(size_t)cap] = prev[(size_t)cap];
    report(tag + "stale_checksum_refused", word_bits(prev[(size_t)cap]) != word_bits(cur[(size_t)cap]) && !ready(torn, cap, k, seq));
    torn = cur;
    torn[(size_t)cap + 1] = prev[(size_t)cap + 1];
    report(tag + "stale_sequence_refused", !ready(torn, cap, k, seq));
  }
  report(tag + "other_count_refused", !ready(cur, cap, k - 1, seq) && !ready(cur, cap, k + 1, seq));
}

}  // namespace

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "pairs")) {
    printf("res_host %d %d\nsteps_res %d %d\nev_host %d %d\n", RES_HOST_CAP, RES_HOST_K, STEPS_RES_CAP, STEPS_RES_K, EV_HOST_SLOTS,
           EV_HOST_SLOTS);
    return 0;
  }
  if (argc == 5 && !strcmp(argv[1], "check")) {
    const int cap = atoi(argv[2]), k = atoi(argv[3]);
    const u64 seq = strtoull(argv[4], nullptr, 10);
    check(cap, k, seq);
    check(cap, k, seq + 1);
    return failures ? 1 : 0;
  }
  fprintf(stderr, "usage: %s pairs | check CAP K SEQ\n", argv[0]);
  return 2;
}
