// Stand-alone check of csrc/scoped.h (built and run by tests/test_scoped_hold.py with -fsanitize=address,undefined; no HIP, no GPU).
#include <cstdio>

#include "scoped.h"

using mimrl::Hold;

static int failures = 0;
#define CHECK(cond) \
  do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

// the engine's error idiom: a macro that returns from the enclosing function
#define MX(expr) \
  do { const int r_ = (expr); if (r_ != 0) return r_; } while (0)

struct Handle {
  int rng_add = 0;
  unsigned side_mask = ~0u;
  bool multi_stream = true;
  const float* text = nullptr;
  int seen_rng = -1;
  unsigned seen_mask = 0;
};

static int launch(Handle& h, int fail) {
  h.seen_rng = h.rng_add;
  h.seen_mask = h.side_mask;
  return fail;
}

static int driver(Handle& h, int fail) {
  Hold sides(h.side_mask, 0x11u);
  {
    Hold key(h.rng_add, 1);
    MX(launch(h, fail));          // returns from inside both scopes
  }
  CHECK(h.rng_add == 0 && h.side_mask == 0x11u);
  return 0;
}

int main() {
  {   // nested holds of ONE variable restore in reverse order
    int v = 1;
    {
      Hold a(v, 2);
      CHECK(v == 2);
      {
        Hold b(v, 3);
        CHECK(v == 3);
        {
          Hold c(v, 4);
          CHECK(v == 4);
        }
        CHECK(v == 3);
      }
      CHECK(v == 2);
    }
    CHECK(v == 1);
  }
  {   // two holds of one scope: the later one goes first
    int v = 1;
    {
      Hold a(v, 2);
      Hold b(v, 3);
      CHECK(v == 3);
    }
    CHECK(v == 1);
  }
  {   // an early return through a macro restores every hold on the way out; the launch saw the held values
    Handle h;
    CHECK(driver(h, 0) == 0);
    CHECK(h.seen_rng == 1 && h.seen_mask == 0x11u);
    CHECK(h.rng_add == 0 && h.side_mask == ~0u);
    h.seen_rng = -1;
    CHECK(driver(h, 7) == 7);
    CHECK(h.seen_rng == 1 && h.seen_mask == 0x11u);
    CHECK(h.rng_add == 0 && h.side_mask == ~0u);
  }
  {   // a pointer and a bool; the value converts to the variable's type
    Handle h;
    const float own[2] = {1.f, 2.f}, other[2] = {3.f, 4.f};
    h.text = own;
    {
      Hold text(h.text, other);
      Hold seq(h.multi_stream, false);
      CHECK(h.text == other && h.text[1] == 4.f && !h.multi_stream);
      {
        Hold none(h.text, nullptr);
        CHECK(h.text == nullptr);
      }
      CHECK(h.text == other);
    }
    CHECK(h.text == own && h.multi_stream);
  }
  if (failures == 0) std::printf("scoped hold ok\n");
  return failures == 0 ? 0 : 1;
}
