// contextrules_flat.hpp -- the context rules of a model in a flat form a lane can evaluate without recursion (lattice.hip scores
// the rules of every final path of a lattice; the host evaluates the same records for anx_debug_contextrule_match).
//
// PatternMatch::parse can only produce a chain of Nots around one atom, or around one Disjunction whose items are chains of Nots
// around atoms (an item cannot contain '|').  Every pattern element therefore is  neg ^ OR_i (neg_i ^ atom_i(id, lexindex))  with the
// atoms Any, NoLexicon, Vocab(id), FromLexicon(bit).  HostModel::add_contextrule keeps the table up to date; a rule that does not
// fit the form (or the widths of the cover word below) clears FlatRules::ok and the model keeps the host decoder.
#pragma once
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define ANX_CF_HD __host__ __device__ inline
#else
#define ANX_CF_HD inline
#endif

namespace anx {

enum : uint32_t { CF_ANY = 0, CF_NOLEXICON = 1, CF_VOCAB = 2, CF_FROMLEXICON = 3, CF_NEG = 0x100u };
struct FlatAtom { uint32_t kind; uint32_t value; };  // kind: CF_* (| CF_NEG: the atom is negated); value: vocabulary id / lexicon bit
struct FlatElem {
  uint32_t atom0;    // first of its atoms
  uint16_t natoms;
  uint8_t neg;       // the disjunction of the atoms is negated
  uint8_t covers;    // a match leaves a result at this position (a rule with tags: only inside one of its tag offsets)
};
struct FlatRule { uint32_t elem0, len; float score; };
// A covered position of a sequence: CF_COVERED | rule << 8 | position in the rule (an uncovered one holds the vocabulary id)
constexpr uint32_t CF_COVERED = 0x80000000u;
constexpr uint32_t CF_MAX_RULES = 1u << 23, CF_MAX_LEN = 255u;

struct FlatRules {
  std::vector<FlatRule> rules;
  std::vector<FlatElem> elems;
  std::vector<FlatAtom> atoms;
  bool ok = true;  // every rule of the model is in the table
};

ANX_CF_HD bool flat_elem_matches(const FlatElem& e, const FlatAtom* atoms, uint32_t id, uint32_t lexindex) {
  bool any = false;
  for (uint32_t i = 0; i < e.natoms && !any; ++i) {
    const FlatAtom a = atoms[e.atom0 + i];
    bool v;
    switch (a.kind & 0xFFu) {
      case CF_ANY: v = true; break;
      case CF_NOLEXICON: v = lexindex == 0u || id == 0u; break;
      case CF_VOCAB: v = id == a.value; break;
      default: v = a.value < 32u && ((lexindex >> a.value) & 1u); break;
    }
    any = v != ((a.kind & CF_NEG) != 0u);
  }
  return any != (e.neg != 0);
}

}  // namespace anx
