// The host relay of the parameter-server handshake page (ps_ops.cpp, kernels/ps_link.h).
//
// A process's GPU can only be given host memory that the process allocated pinned itself
// (hipHostMalloc); memory it merely maps - the POSIX shm page the ps task and its workers share -
// cannot be registered for device access everywhere.  So every process keeps two copies of the
// page: the shared mapping, which the hosts read and write, and a pinned page of its own, which
// its GPU reads and writes.  One relay thread per process moves each group of handshake words
// between the two, in the direction the group travels:
//
//   request / bucket words   worker GPU -> worker pinned -(worker relay)-> shared -> ps host
//   reply words              ps GPU -> ps pinned -(ps relay)-> shared -> worker host
//                                                      shared -(worker relay)-> worker pinned -> worker GPU
//
// A group is its payload words and the sequence word its writer stores last.  The relay reads the
// sequence word first (acquire), then copies the payload, then stores the sequence word (release),
// so a reader of the copy sees the payload of that sequence number - the order the writer kept.
// A group has one writer, and its writer only writes it again after the answer to the previous
// write came back through the relays, so a payload never changes under a copy.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../kernels/ps_link.h"

namespace dtfe {

struct PsHop {
  int seq, lo, n;  // sequence word, payload words [lo, lo + n)
  bool from_ps;    // written by the ps's GPU (else by the worker's)
};
constexpr PsHop PS_HOPS[] = {
    {PS_REQ_SEQ, PS_REQ_KIND, 2, false},
    {PS_REP_SEQ, PS_REP_GS, 3, true},
    {PS_BKT_BASE + 0, PS_BKT_BASE + 1, 2, false},
    {PS_BKT_BASE + 3, PS_BKT_BASE + 4, 2, false},
    {PS_BKT_BASE + 6, PS_BKT_BASE + 7, 2, false},
    {PS_BKT_BASE + 9, PS_BKT_BASE + 10, 2, false},
};
constexpr size_t PS_NHOPS = sizeof(PS_HOPS) / sizeof(PS_HOPS[0]);
static_assert(PS_NHOPS == 2 + PS_MAX_BUCKETS, "one hop per bucket");

// One pass over `nslots` worker slots of a page: `shared` is the mapping every process has,
// `pinned` this process's own page, `ps` says whether this process is the ps task.  `seen`
// (nslots * PS_NHOPS, zero at first) holds the sequence numbers already moved.  Returns whether
// anything moved.  The ps moves only what its GPU writes (its host reads the requests in the shared
// page itself); a worker moves its GPU's words out and the replies in.  Slots of other workers
// never change in a worker's pinned page, so nothing of them goes out.
inline bool ps_relay_pass(uint64_t* shared, uint64_t* pinned, size_t nslots, bool ps, std::vector<uint64_t>& seen) {
  bool any = false;
  for (size_t w = 0; w < nslots; ++w) {
    uint64_t* sh = shared + w * PS_SLOT_WORDS;
    uint64_t* pn = pinned + w * PS_SLOT_WORDS;
    // A worker's GPU announces a push's buckets before it sends the request, and the ps looks for
    // the buckets of a request when it sees the request: the request number is read first and
    // moved last, so the shared page never shows a request ahead of its buckets.
    uint64_t now[PS_NHOPS];
    for (size_t h = 0; h < PS_NHOPS; ++h) {
      const PsHop& hop = PS_HOPS[h];
      now[h] = __atomic_load_n((hop.from_ps == ps ? pn : sh) + hop.seq, __ATOMIC_ACQUIRE);
    }
    for (size_t h = PS_NHOPS; h-- > 0;) {
      const PsHop& hop = PS_HOPS[h];
      if (ps && !hop.from_ps) continue;
      const bool out = hop.from_ps == ps;  // this process's GPU writes the group
      const uint64_t* src = out ? pn : sh;
      uint64_t* dst = out ? sh : pn;
      uint64_t& last = seen[w * PS_NHOPS + h];
      if (now[h] == last) continue;
      for (int i = hop.lo; i < hop.lo + hop.n; ++i)
        __atomic_store_n(dst + i, __atomic_load_n(src + i, __ATOMIC_RELAXED), __ATOMIC_RELAXED);
      __atomic_store_n(dst + hop.seq, now[h], __ATOMIC_RELEASE);
      last = now[h];
      any = true;
    }
  }
  return any;
}

}  // namespace dtfe
