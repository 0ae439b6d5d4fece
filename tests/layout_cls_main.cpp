// Stand-alone host program (CPU tier, built with -fsanitize=address,undefined by tests/test_class_loss_host.py): the parameter layout of a
// classification head through the C ABI -- mimrl_layout_count / mimrl_layout_entry at num_class 1, 7 and 9 on a zero-initialised mimrl_cfg
// with tiny_sep's shape.  Prints "layout cls ok" when every check held.
#include <cstdio>
#include <cstring>
#include <string>

#include "../include/mimrl.h"

static int failures = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

static mimrl_cfg tiny(int num_class) {
  mimrl_cfg c;
  std::memset(&c, 0, sizeof c);
  c.batch = 8; c.seq_len = 6; c.time_len = 6; c.d_t = 768; c.d_a = 74; c.d_v = 35; c.d_common = 128;
  c.n_blocks = 2;
  const int cube[2][3] = {{6, 3, 128}, {4, 3, 128}};
  for (int i = 0; i < 2; ++i) {
    for (int ax = 0; ax < 3; ++ax) { c.d_hiddens[i][ax] = cube[i][ax]; c.d_outs[i][ax] = cube[i][ax]; }
    c.res_project[i] = 1;
  }
  c.bias = 1; c.activation = MIMRL_ACT_GELU; c.k_neighbor = 2; c.bank_capacity = 40;
  c.num_class = num_class;
  return c;
}

// -> index of `want`, its dims in d0 / d1 / nd and offset in off; -1 when absent
static int find(const mimrl_cfg& c, const char* want, int* nd, int* d0, int* d1, int64_t* off) {
  const int n = mimrl_layout_count(&c);
  for (int i = 0; i < n; ++i) {
    char name[256];
    int group = -1;
    if (mimrl_layout_entry(&c, i, name, (int)sizeof name, &group, off, nd, d0, d1) != MIMRL_OK) return -1;
    if (std::strcmp(name, want) == 0) { CHECK(group == MIMRL_GROUP_MAIN); return i; }
  }
  return -1;
}

int main() {
  int64_t main_floats[3] = {0, 0, 0};
  const int classes[3] = {0, 1, 7};
  int count1 = 0;
  for (int q = 0; q < 3; ++q) {
    const mimrl_cfg c = tiny(classes[q]);
    const int want = classes[q] >= 2 ? classes[q] : 1;
    const int n = mimrl_layout_count(&c);
    CHECK(n > 0);
    if (q == 0) count1 = n;
    CHECK(n == count1);                                   // the same tensors at every class count
    int nd = 0, d0 = 0, d1 = 0;
    int64_t off = -1;
    CHECK(find(c, "classifier.0.weight", &nd, &d0, &d1, &off) >= 0);
    CHECK(nd == 2 && d0 == want && d1 == 128 && off >= 0 && off % 64 == 0);
    CHECK(find(c, "classifier.0.bias", &nd, &d0, &d1, &off) >= 0);
    CHECK(nd == 1 && d0 == want && off >= 0 && off % 64 == 0);
    char small[4];                                        // a short name buffer is truncated and terminated, not overrun
    CHECK(mimrl_layout_entry(&c, 0, small, (int)sizeof small, nullptr, nullptr, nullptr, nullptr, nullptr) == MIMRL_OK);
    CHECK(std::strlen(small) == 3);
    CHECK(mimrl_layout_entry(&c, n, small, (int)sizeof small, nullptr, nullptr, nullptr, nullptr, nullptr) == MIMRL_ERR_ARG);
    main_floats[q] = mimrl_bucket_floats(&c, MIMRL_GROUP_MAIN);
    const mimrl_cfg one = tiny(1);
    CHECK(mimrl_bucket_floats(&c, MIMRL_GROUP_CRITIC) == mimrl_bucket_floats(&one, MIMRL_GROUP_CRITIC));
  }
  CHECK(main_floats[0] == main_floats[1]);                // 0 and 1: the one-output head
  CHECK(main_floats[2] == main_floats[1] + 6 * 128);      // a [7, 128] weight in place of [1, 128]; either bias fills one 64-float slot
  for (int bad : {MIMRL_MAX_CLASSES + 1, -1}) {
    const mimrl_cfg c = tiny(bad);
    char name[64];
    CHECK(mimrl_layout_count(&c) == MIMRL_ERR_ARG);
    CHECK(std::string(mimrl_last_error()).find("num_class") != std::string::npos);
    CHECK(mimrl_layout_entry(&c, 0, name, (int)sizeof name, nullptr, nullptr, nullptr, nullptr, nullptr) == MIMRL_ERR_ARG);
    CHECK(mimrl_bucket_floats(&c, MIMRL_GROUP_MAIN) == MIMRL_ERR_ARG);
  }
  if (failures == 0) std::printf("layout cls ok\n");
  return failures == 0 ? 0 : 1;
}
