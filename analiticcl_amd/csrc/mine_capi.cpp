// mine_capi.cpp -- anx_mine_confusables / anx_mine_confusables_packed: from (observed, correct) string pairs to the change sites of
// their edit scripts and the table of distinct sites in confusable-list notation (src/confusables.rs: the patterns a confusable list
// holds; src/lib.rs:1733-1756: how a list weighs a row).  The scripts, the sites' keys and the histogram are mine.hip's; this file owns
// the argument checks, the chunking (at most 2^20 pairs, as pairs_capi.cpp), the texts of the distinct sites (built from the
// representatives' pairs out of the caller's strings), the pairs the device hands back (scripted with the host core, confusables.cpp
// edit_script_ops), the merge of the chunks' tables by text and the table's order.  Host work is O(distinct patterns + host pairs) plus
// the staging of the strings; the site records stay on the device until their final pattern indices are known and come back in place.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "mine.h"
#include "pair_spans.h"

const anx::HostModel& anx_host_of(const anx_model* m);
const anx::DeviceLexicon* anx_replica_of(const anx_model* m, size_t i);
int anx_fail(int code, const std::string& msg);

namespace {
std::atomic<uint64_t> g_stats[anx::MINE_NCTR];
std::atomic<size_t> g_chunk{anx::PAIRS_CHUNK};

struct Result {
  anx_mine_result pub;  // (first: anx_mine_result_free casts back)
  std::string text;
  std::vector<uint64_t> text_off, count, sites, site_off;
  std::vector<uint32_t> flags;
  std::vector<anx_mine_site> site;
};

typedef std::vector<uint32_t> CP;
void decode(const anx::PairSpan& s, CP& out) {
  out.clear();
  for (size_t i = 0; i < s.len;) {
    int l;
    out.push_back(anx::utf8_decode_at(s.p + i, s.len - i, &l));
    i += (size_t)l;
  }
}
void put_utf8(std::string& out, uint32_t c) {
  if (c < 0x80) out.push_back((char)c);
  else if (c < 0x800) { out.push_back((char)(0xC0 | (c >> 6))); out.push_back((char)(0x80 | (c & 0x3F))); }
  else if (c < 0x10000) { out.push_back((char)(0xE0 | (c >> 12))); out.push_back((char)(0x80 | ((c >> 6) & 0x3F))); out.push_back((char)(0x80 | (c & 0x3F))); }
  else { out.push_back((char)(0xF0 | (c >> 18))); out.push_back((char)(0x80 | ((c >> 12) & 0x3F))); out.push_back((char)(0x80 | ((c >> 6) & 0x3F))); out.push_back((char)(0x80 | (c & 0x3F))); }
}
// one instruction; *bad: a character the list parser cannot take
void put_ins(std::string& out, char op, const uint32_t* s, size_t n, bool* bad) {
  out.push_back(op);
  out.push_back('[');
  for (size_t i = 0; i < n; ++i) {
    if (s[i] == '[' || s[i] == ']' || s[i] == '|') *bad = true;
    put_utf8(out, s[i]);
  }
  out.push_back(']');
}

// the merged table while the chunks come in
struct Table {
  std::unordered_map<std::string, uint32_t> idx;
  std::vector<const std::string*> text;  // (keys of idx: stable addresses)
  std::vector<uint64_t> count, sites;
  std::vector<uint32_t> flags;
  uint32_t add(const std::string& t, bool bad, uint64_t c, uint64_t s) {
    auto it = idx.find(t);
    if (it == idx.end()) {
      it = idx.emplace(t, (uint32_t)text.size()).first;
      text.push_back(&it->first);
      count.push_back(0);
      sites.push_back(0);
      flags.push_back(bad ? (uint32_t)ANX_MINE_UNREPRESENTABLE : 0u);
    }
    count[it->second] += c;
    sites[it->second] += s;
    return it->second;
  }
};

// a pair on the host: its sites left to right, straight from the script's instructions (any shape)
void host_pair(const anx::PairSpan& a, const anx::PairSpan& b, uint32_t pair, uint64_t weight, uint32_t context, bool anchors, Table& T,
               std::vector<anx_mine_site>* out, uint64_t* nsites, uint64_t* odd) {
  static thread_local CP ca, cb;
  static thread_local std::vector<anx::ScriptOp> ops;
  static thread_local std::string text;
  decode(a, ca);
  decode(b, cb);
  anx::edit_script_ops(ca.data(), ca.size(), cb.data(), cb.size(), ops);
  size_t apos = 0, bpos = 0;
  bool pair_odd = false;
  for (size_t i = 0; i < ops.size();) {
    if (ops[i].op == '=') { apos += ops[i].len; bpos += ops[i].len; ++i; continue; }
    size_t j = i;
    while (j < ops.size() && ops[j].op != '=') ++j;
    if (!(j - i == 1 || (j - i == 2 && ops[i].op == '-' && ops[i + 1].op == '+'))) pair_odd = true;
    const bool first = i == 0, last = j == ops.size();
    bool bad = false;
    text.clear();
    if (anchors && first) text.push_back('^');
    if (context && i > 0) {
      const size_t k = std::min<size_t>(context, ops[i - 1].len);
      put_ins(text, '=', ca.data() + apos - k, k, &bad);
    }
    anx_mine_site s{};
    s.pair = pair; s.a_pos = (uint32_t)apos; s.b_pos = (uint32_t)bpos;
    for (size_t k = i; k < j; ++k) {
      if (ops[k].op == '-') { put_ins(text, '-', ca.data() + apos, ops[k].len, &bad); apos += ops[k].len; s.a_len += ops[k].len; }
      else { put_ins(text, '+', cb.data() + bpos, ops[k].len, &bad); bpos += ops[k].len; s.b_len += ops[k].len; }
    }
    if (context && j < ops.size()) {
      const size_t k = std::min<size_t>(context, ops[j].len);
      put_ins(text, '=', ca.data() + apos, k, &bad);
    }
    if (anchors && last) text.push_back('$');
    s.flags = (first ? (uint32_t)ANX_MINE_SITE_FIRST : 0u) | (last ? (uint32_t)ANX_MINE_SITE_LAST : 0u);
    s.pattern = T.add(text, bad, weight, 1);
    if (out) out->push_back(s);
    ++*nsites;
    i = j;
  }
  if (pair_odd) ++*odd;
}

// the text of a device row from its representative's pair
uint32_t add_row(const anx::MineRow& r, const anx::PairSpan& a, const anx::PairSpan& b, bool anchors, Table& T) {
  static thread_local CP ca, cb;
  static thread_local std::string text;
  decode(a, ca);
  decode(b, cb);
  const uint32_t a_pos = r.pos & 0xFFu, a_len = (r.pos >> 8) & 0xFFu, b_pos = (r.pos >> 16) & 0xFFu, b_len = r.pos >> 24;
  const uint32_t lc = r.meta & 0xFu, rc = (r.meta >> 4) & 0xFu;
  bool bad = false;
  text.clear();
  if (a_pos + a_len + rc > ca.size() || lc > a_pos || b_pos + b_len > cb.size()) return 0xFFFFFFFFu;  // (a record the strings do not bear out)
  if (anchors && (r.meta & 0x100u)) text.push_back('^');
  if (lc) put_ins(text, '=', ca.data() + a_pos - lc, lc, &bad);
  if (a_len) put_ins(text, '-', ca.data() + a_pos, a_len, &bad);
  if (b_len) put_ins(text, '+', cb.data() + b_pos, b_len, &bad);
  if (rc) put_ins(text, '=', ca.data() + a_pos + a_len, rc, &bad);
  if (anchors && (r.meta & 0x200u)) text.push_back('$');
  return T.add(text, bad, r.count, r.sites);
}

struct ChunkState {
  size_t lo = 0, n = 0;
  anx::MineChunk* dev = nullptr;
  std::vector<uint32_t> rowmap;           // chunk pattern index -> row of Table
  std::vector<uint32_t> host_pairs;       // chunk-relative, ascending
  std::vector<anx_mine_site> host_sites;  // of host_pairs, in that order
};
struct Chunks {
  std::vector<ChunkState> v;
  ~Chunks() { for (ChunkState& c : v) anx::mine_chunk_free(c.dev); }
};

int run(const anx_model* m, const std::vector<anx::PairSpan>& a, const std::vector<anx::PairSpan>& b, const uint32_t* count, const anx_mine_params* p,
        anx_mine_result** out) {
  const size_t n = a.size();
  const bool host_only = anx::switches().mine_host != 0, anchors = p->anchors != 0, want_sites = p->no_sites == 0;
  const uint32_t context = p->context;
  const size_t chunk = g_chunk.load(std::memory_order_relaxed);
  Table T;
  Chunks cs;
  uint64_t st[anx::MINE_NCTR] = {};
  uint64_t &up = st[6], &down = st[7], odd_again = 0;  // (odd_again: a pair the device handed back for its shape is counted there)
  size_t total_sites = 0;
  for (size_t lo = 0; lo < n; lo += chunk) {
    cs.v.emplace_back();
    ChunkState& c = cs.v.back();
    c.lo = lo;
    c.n = std::min(chunk, n - lo);
    if (host_only) {
      c.host_pairs.resize(c.n);
      for (size_t i = 0; i < c.n; ++i) c.host_pairs[i] = (uint32_t)i;
    } else {
      std::vector<anx::MineRow> rows;
      std::string err;
      const int rc = anx::mine_chunk_run(anx_replica_of(m, 0), a.data() + lo, b.data() + lo, count ? count + lo : nullptr, c.n, context, anchors, want_sites,
                                         &c.dev, rows, c.host_pairs, st, &up, &down, err);
      if (rc) return anx_fail(rc, err);
      c.rowmap.resize(rows.size());
      T.idx.reserve(T.idx.size() + rows.size());
      for (size_t r = 0; r < rows.size(); ++r) {
        if (rows[r].pair >= c.n) return anx_fail(ANX_EINVAL, "mine: inconsistent device table");
        c.rowmap[r] = add_row(rows[r], a[lo + rows[r].pair], b[lo + rows[r].pair], anchors, T);
        if (c.rowmap[r] == 0xFFFFFFFFu) return anx_fail(ANX_EINVAL, "mine: inconsistent device table");
        st[2] += rows[r].sites;
        total_sites += rows[r].sites;
      }
      st[0] += c.n - c.host_pairs.size();
    }
    uint64_t hs = 0;
    for (uint32_t i : c.host_pairs)
      host_pair(a[lo + i], b[lo + i], (uint32_t)(lo + i), count ? count[lo + i] : 1u, context, anchors, T, want_sites ? &c.host_sites : nullptr, &hs,
                host_only ? &st[5] : &odd_again);
    st[1] += c.host_pairs.size();
    st[2] += hs;
    total_sites += hs;
  }
  st[3] = T.text.size();
  // ---- the table's order: count descending, sites descending, text bytes ascending ----
  const size_t D = T.text.size();
  std::vector<uint32_t> order(D), final_of(D);
  for (size_t i = 0; i < D; ++i) order[i] = (uint32_t)i;
  std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
    if (T.count[x] != T.count[y]) return T.count[x] > T.count[y];
    if (T.sites[x] != T.sites[y]) return T.sites[x] > T.sites[y];
    return *T.text[x] < *T.text[y];  // (std::string compares as unsigned bytes, the shorter of two with a common prefix first)
  });
  Result* R = new Result();
  R->text_off.resize(D + 1);
  R->count.resize(D);
  R->sites.resize(D);
  R->flags.resize(D);
  for (size_t k = 0; k < D; ++k) {
    const uint32_t x = order[k];
    final_of[x] = (uint32_t)k;
    R->text_off[k] = R->text.size();
    R->text += *T.text[x];
    R->count[k] = T.count[x];
    R->sites[k] = T.sites[x];
    R->flags[k] = T.flags[x];
  }
  R->text_off[D] = R->text.size();
  // ---- the site list: the device's records come back in place, the host pairs' are spliced in ----
  if (want_sites) {
    R->site.resize(total_sites);
    R->site_off.resize(n + 1);
    size_t base = 0;
    std::vector<uint32_t> remap, off;
    std::vector<anx_mine_site> tmp;
    for (ChunkState& c : cs.v) {
      const size_t nd = c.dev ? anx::mine_chunk_sites(c.dev) : 0;
      off.assign(c.n + 1, 0);
      anx_mine_site* dst = R->site.data() + base;
      const bool splice = nd && !c.host_sites.empty();
      if (nd) {
        remap.resize(c.rowmap.size());
        for (size_t r = 0; r < remap.size(); ++r) remap[r] = final_of[c.rowmap[r]];
        if (splice) { tmp.resize(nd); dst = tmp.data(); }
        std::string err;
        if (base + nd + c.host_sites.size() > total_sites) { delete R; return anx_fail(ANX_EINVAL, "mine: inconsistent site totals"); }
        const int rc = anx::mine_chunk_emit(c.dev, remap.data(), remap.size(), (uint32_t)c.lo, dst, off.data(), &down, err);
        if (rc) { delete R; return anx_fail(rc, err); }
      }
      for (anx_mine_site& s : c.host_sites) s.pattern = final_of[s.pattern];
      if (c.host_sites.empty()) {
        for (size_t i = 0; i <= c.n; ++i) R->site_off[c.lo + i] = base + off[i];
        base += nd;
        continue;
      }
      // host pairs have no sites on the device: the device's run of sites between two host pairs moves as one block
      anx_mine_site* o = R->site.data() + base;
      size_t w = 0, hp = 0, hsite = 0, prev = 0;  // w: written; prev: first pair of the pending device block
      auto flush = [&](size_t upto) {             // device sites of pairs [prev, upto)
        const size_t cnt = off[upto] - off[prev];
        if (cnt) memcpy(o + w, tmp.data() + off[prev], cnt * sizeof(anx_mine_site));
        for (size_t i = prev; i < upto; ++i) R->site_off[c.lo + i] = base + w + (off[i] - off[prev]);
        w += cnt;
        prev = upto;
      };
      for (; hp < c.host_pairs.size(); ++hp) {
        const size_t i = c.host_pairs[hp];
        if (nd) flush(i);
        else for (size_t k = prev; k < i; ++k) R->site_off[c.lo + k] = base + w;
        R->site_off[c.lo + i] = base + w;
        while (hsite < c.host_sites.size() && c.host_sites[hsite].pair == c.lo + i) o[w++] = c.host_sites[hsite++];
        prev = i + 1;
      }
      if (nd) flush(c.n);
      else for (size_t k = prev; k < c.n; ++k) R->site_off[c.lo + k] = base + w;
      base += w;
      R->site_off[c.lo + c.n] = base;
    }
    R->site_off[n] = base;
    if (base != total_sites) { delete R; return anx_fail(ANX_EINVAL, "mine: inconsistent site totals"); }
  }
  R->pub.n_patterns = D;
  R->pub.text = R->text.data();
  R->pub.text_off = R->text_off.data();
  R->pub.count = R->count.data();
  R->pub.sites = R->sites.data();
  R->pub.flags = R->flags.data();
  R->pub.n_pairs = n;
  R->pub.n_sites = total_sites;
  R->pub.site_off = want_sites ? R->site_off.data() : nullptr;
  R->pub.site = want_sites ? R->site.data() : nullptr;
  for (int k = 0; k < anx::MINE_NCTR; ++k) g_stats[k].fetch_add(st[k], std::memory_order_relaxed);
  *out = &R->pub;
  return ANX_OK;
}

int check_call(const anx_model* m, const void* a, const void* b, size_t n, const anx_mine_params* p, anx_mine_result** out) {
  if (!m || !p || !out) return anx_fail(ANX_EINVAL, "NULL argument");
  *out = nullptr;
  if (n && (!a || !b)) return anx_fail(ANX_EINVAL, "NULL argument");
  if (p->context > anx::MINE_MAX_CONTEXT) return anx_fail(ANX_EINVAL, "mine: context beyond 8 code points");
  if (n >= ((size_t)1 << 32)) return anx_fail(ANX_ELIMIT, "mine: 2^32 pairs or more: split the call");
  if (n && !anx::switches().mine_host) {
    if (!anx_host_of(m).built) return anx_fail(ANX_ENOTBUILT, "Model has not been built yet! Call build() before mine_confusables()");
    if (!anx_replica_of(m, 0)) return anx_fail(ANX_ENODEVICE, "model is not resident on a device (no HIP device / anx_model_to_device not called)");
  }
  return ANX_OK;
}
}  // namespace

extern "C" {
void anx_default_mine_params(anx_mine_params* out) {
  if (out) memset(out, 0, sizeof *out);
}
int anx_mine_confusables(const anx_model* m, const char* const* a, const char* const* b, const uint32_t* count, size_t n, const anx_mine_params* p,
                         anx_mine_result** out) {
  if (int rc = check_call(m, a, b, n, p, out)) return rc;
  std::vector<anx::PairSpan> sa, sb;
  if (!anx::spans_of_pointers(a, n, sa) || !anx::spans_of_pointers(b, n, sb)) return anx_fail(ANX_EINVAL, "NULL string");
  return run(m, sa, sb, count, p, out);
}
int anx_mine_confusables_packed(const anx_model* m, const char* blob_a, size_t len_a, const char* blob_b, size_t len_b, const uint32_t* count, size_t n,
                                const anx_mine_params* p, anx_mine_result** out) {
  if (int rc = check_call(m, blob_a, blob_b, n, p, out)) return rc;
  if (len_a >= ((size_t)1 << 32) || len_b >= ((size_t)1 << 32)) return anx_fail(ANX_ELIMIT, "packed pairs exceed 4 GB per blob: split the call");
  std::vector<anx::PairSpan> sa, sb;
  if (!anx::spans_of(blob_a, len_a, n, sa) || !anx::spans_of(blob_b, len_b, n, sb)) return anx_fail(ANX_EINVAL, "packed inputs hold fewer strings than announced");
  return run(m, sa, sb, count, p, out);
}
void anx_mine_result_free(anx_mine_result* r) {
  if (r) delete reinterpret_cast<Result*>(r);
}
int anx_format_confusable_list(const anx_mine_result* r, double weight, uint64_t min_count, char** text) {
  if (!r || !text) return anx_fail(ANX_EINVAL, "NULL argument");
  std::string out;
  char w[40];
  snprintf(w, sizeof w, "%.17g", weight);
  for (size_t k = 0; k < r->n_patterns; ++k) {
    if (r->count[k] < min_count || (r->flags[k] & ANX_MINE_UNREPRESENTABLE)) continue;
    out.append(r->text + r->text_off[k], r->text_off[k + 1] - r->text_off[k]);
    out.push_back('\t');
    out += w;
    out.push_back('\n');
  }
  char* s = static_cast<char*>(malloc(out.size() + 1));
  if (!s) return anx_fail(ANX_EINVAL, "out of host memory");
  memcpy(s, out.c_str(), out.size() + 1);
  *text = s;
  return ANX_OK;
}
int anx_debug_mine_stats(uint64_t* out) {
  if (!out) return anx_fail(ANX_EINVAL, "NULL argument");
  for (int k = 0; k < anx::MINE_NCTR; ++k) out[k] = g_stats[k].load(std::memory_order_relaxed);
  return ANX_OK;
}
int anx_debug_mine_chunk(size_t chunk) {
  if (chunk > anx::PAIRS_CHUNK) return anx_fail(ANX_EINVAL, "mine: chunk size outside 1 .. 2^20");
  g_chunk.store(chunk ? chunk : anx::PAIRS_CHUNK, std::memory_order_relaxed);
  return ANX_OK;
}
}  // extern "C"
