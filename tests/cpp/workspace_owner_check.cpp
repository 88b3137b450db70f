// hfg::WorkspaceOwner with counting dummy workspaces, for builds with -fsanitize=address,undefined and with
// -fsanitize=thread (tests/test_workspace_owner_cpu.py): construction on first use, the accessor that never creates, a
// set-up that throws, destruction with the owner, and two threads that each hammer an owner of their own.
#include "../../helfem_amd/csrc/hip/workspace_owner.h"
#include <atomic>
#include <cstdio>
#include <stdexcept>
#include <thread>
#include <vector>

static std::atomic<int> g_made(0), g_gone(0);

template <int TAG>
struct Dummy : hfg::Workspace {
  std::vector<int> heap;  // something for the sanitizer to track
  int setups = 0;
  const void *owner = nullptr;
  Dummy() : heap(17, TAG) { g_made++; }
  ~Dummy() override { g_gone++; }
};
typedef hfg::WorkspaceOwner<3> Owner;

#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("owner WRONG: %s (line %d)\n", #cond, __LINE__);    \
      return false;                                              \
    }                                                            \
  } while (0)

static bool first_use() {
  const int made0 = g_made, gone0 = g_gone;
  {
    Owner o;
    CHECK(o.find<Dummy<0> >(0) == nullptr && o.find<Dummy<1> >(1) == nullptr);
    CHECK(g_made == made0);  // find never creates
    Dummy<0> &a = o.get<Dummy<0> >(0, [](Dummy<0> &w) { w.setups++; });
    CHECK(g_made == made0 + 1 && a.setups == 1 && a.heap.size() == 17);
    Dummy<0> &b = o.get<Dummy<0> >(0, [](Dummy<0> &w) { w.setups++; });
    CHECK(&a == &b && b.setups == 1 && g_made == made0 + 1);  // the same object, set up once
    CHECK(o.find<Dummy<0> >(0) == &a);
    CHECK(o.find<Dummy<1> >(1) == nullptr);  // the other slots are untouched
    Dummy<1> &c = o.get<Dummy<1> >(1);       // no set-up
    CHECK(c.setups == 0 && c.heap[0] == 1 && o.find<Dummy<1> >(1) == &c && g_made == made0 + 2);
    CHECK(g_gone == gone0);
  }
  CHECK(g_gone == gone0 + 2);
  return true;
}

static bool throwing_setup() {
  const int made0 = g_made, gone0 = g_gone;
  Owner o;
  bool caught = false;
  try {
    o.get<Dummy<2> >(2, [](Dummy<2> &) { throw std::runtime_error("upload failed"); });
  } catch (const std::runtime_error &) {
    caught = true;
  }
  CHECK(caught && g_made == made0 + 1 && g_gone == gone0 + 1);  // built once, destroyed once
  CHECK(o.find<Dummy<2> >(2) == nullptr);                        // and not published
  Dummy<2> &w = o.get<Dummy<2> >(2, [](Dummy<2> &d) { d.setups++; });
  CHECK(g_made == made0 + 2 && g_gone == gone0 + 1 && w.setups == 1 && o.find<Dummy<2> >(2) == &w);
  o.drop_all();
  CHECK(g_gone == gone0 + 2 && o.find<Dummy<2> >(2) == nullptr);
  o.drop_all();  // nothing left to destroy
  CHECK(g_gone == gone0 + 2);
  return true;
}

static bool two_owners() {
  const int made0 = g_made, gone0 = g_gone;
  {
    Owner *p = new Owner(), *q = new Owner();
    Dummy<0> &a = p->get<Dummy<0> >(0), &b = q->get<Dummy<0> >(0);
    CHECK(&a != &b);
    p->get<Dummy<1> >(1);
    p->get<Dummy<2> >(2);
    CHECK(g_made == made0 + 4);
    delete p;  // every workspace of p exactly once, none of q's
    CHECK(g_gone == gone0 + 3 && q->find<Dummy<0> >(0) == &b && b.heap[16] == 0);
    // an owner at a recycled address starts empty
    Owner *r = new Owner();
    CHECK(r->find<Dummy<0> >(0) == nullptr && r->find<Dummy<1> >(1) == nullptr && r->find<Dummy<2> >(2) == nullptr);
    delete r;
    delete q;
  }
  CHECK(g_made == made0 + 4 && g_gone == gone0 + 4);
  return true;
}

// one owner per thread, as one context per host thread: no lock, and nothing for a race detector to find
static void hammer(int seed, long *sum) {
  for (int round = 0; round < 200; round++) {
    Owner o;
    for (int i = 0; i < 50; i++) {
      Dummy<0> &a = o.get<Dummy<0> >(0, [&](Dummy<0> &w) { w.owner = &o; });
      Dummy<1> &b = o.get<Dummy<1> >(1, [&](Dummy<1> &w) { w.owner = &o; });
      if (a.owner != &o || b.owner != &o || o.find<Dummy<0> >(0) != &a) *sum = -1000000000;
      a.heap[(seed + i) % 17]++;
      *sum += a.heap[(seed + i) % 17] + b.heap[i % 17];
      if (i == 25) o.drop_all();
    }
  }
}

static bool two_threads() {
  const int made0 = g_made, gone0 = g_gone;
  long s1 = 0, s2 = 0, s3 = 0;
  std::thread t1(hammer, 3, &s1), t2(hammer, 3, &s2);
  t1.join();
  t2.join();
  hammer(3, &s3);
  CHECK(s1 == s3 && s2 == s3 && s3 > 0);  // each thread saw only its own workspaces
  CHECK(g_made - made0 == 3 * 200 * 4 && g_gone - gone0 == 3 * 200 * 4);
  return true;
}

int main() {
  const bool ok = first_use() && throwing_setup() && two_owners() && two_threads() && g_made == g_gone;
  printf(ok ? "owner ok\n" : "owner WRONG\n");
  return ok ? 0 : 1;
}
