// Workspaces owned by the object they serve.  A stage of the eigensolver keeps its scratch buffers, cached task lists and
// pinned status words in its context (hfg_ctx), a Fock or exchange build in its table set (hfg_dev_tables); each has one
// slot here and dies with its owner.  Nothing is looked up by a pointer and nothing is shared between owners, so "one
// context per host thread" needs no lock.  Host only: no HIP call in this file (tests/cpp/workspace_owner_check.cpp
// includes nothing else).
#pragma once
#include <memory>
#include <utility>

namespace hfg {

struct Workspace {
  virtual ~Workspace() {}
};

// the slots of a context and of a table set; the structs stay in the files named
enum CtxSlot { WS_EIG, WS_DC, WS_STSEL, WS_TRD, WS_TRDP, WS_CUHF, WS_OCC, WS_CTX_SLOTS };  // eig.hip, dc.hip, stsel.hip, trd.hip, trdp.hip, cuhf_dev.hip, occupy.hip
enum TableSlot { WS_FOCK, WS_EX, WS_EXLR, WS_COULOMB_BATCH, WS_EXLR_BATCH, WS_TABLE_SLOTS };  // fock.hip, exchange.hip, exchange_lr.hip, fock.hip, exchange_lr.hip

template <int NSLOTS>
struct WorkspaceOwner {
  std::unique_ptr<Workspace> slot[NSLOTS];

  /// the slot's workspace, or null when nothing has built it yet; never creates
  template <class W>
  W *find(int i) const {
    return static_cast<W *>(slot[i].get());
  }
  /// the slot's workspace; the first call constructs a W and runs setup(W &) on it.  The slot is filled only after setup
  /// has returned: one that throws destroys the new workspace and leaves the slot empty for the next call.
  template <class W, class Setup>
  W &get(int i, Setup &&setup) {
    if (!slot[i]) {
      std::unique_ptr<W> w(new W());
      setup(*w);
      slot[i] = std::move(w);
    }
    return static_cast<W &>(*slot[i]);
  }
  template <class W>
  W &get(int i) {
    return get<W>(i, [](W &) {});
  }
  /// destroys every workspace, in slot order
  void drop_all() {
    for (auto &s : slot) s.reset();
  }
};

}  // namespace hfg
