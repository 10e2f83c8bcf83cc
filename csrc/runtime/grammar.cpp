#include "grammar.h"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <functional>
#include <set>
#include <stdexcept>

#include "tokenizer.h"

namespace mp {

// ------------------------------------------------------------------ character sets
static void merge_ranges(std::vector<std::pair<uint32_t, uint32_t>>& r) {
  std::sort(r.begin(), r.end());
  size_t o = 0;
  for (size_t i = 0; i < r.size(); ++i) {
    if (o && (uint64_t)r[i].first <= (uint64_t)r[o - 1].second + 1) r[o - 1].second = std::max(r[o - 1].second, r[i].second);
    else r[o++] = r[i];
  }
  r.resize(o);
}

bool Grammar::Elem::match(uint32_t cp) const {
  bool in = false;
  for (const auto& [a, b] : ranges) {
    if (cp < a) break;
    if (cp <= b) { in = true; break; }
  }
  return in != neg;
}

bool Grammar::Elem::match_any_in(uint32_t lo, uint32_t hi) const {
  if (!neg) {
    for (const auto& [a, b] : ranges)
      if (a <= hi && b >= lo) return true;
    return false;
  }
  // negated: some code point of [lo, hi] lies outside every range (ranges are sorted and merged)
  uint64_t need = lo;
  for (const auto& [a, b] : ranges) {
    if (b < need) continue;
    if (a > need) return true;
    need = (uint64_t)b + 1;
    if (need > hi) return false;
  }
  return need <= hi;
}

// ------------------------------------------------------------------ parser
struct GrammarParser {
  const std::string& src;
  Grammar& g;
  size_t pos = 0;
  std::map<std::string, int> ids;
  std::vector<char> defined;
  std::vector<std::string> owner;    // the user rule a (synthesized) rule belongs to
  std::vector<size_t> where;         // definition (or first reference) offset
  std::string cur = "root";
  int n_synth = 0, depth = 0;
  size_t n_elems = 0;

  GrammarParser(const std::string& s, Grammar& gr) : src(s), g(gr) {}

  [[noreturn]] void fail(const std::string& rule, size_t at, const std::string& msg) const {
    size_t line = 1, col = 1;
    for (size_t i = 0; i < at && i < src.size(); ++i) {
      if (src[i] == '\n') { ++line; col = 1; }
      else ++col;
    }
    throw std::runtime_error("grammar: rule \"" + rule + "\" (line " + std::to_string(line) + ", column " +
                             std::to_string(col) + "): " + msg);
  }
  [[noreturn]] void fail(const std::string& msg) const { fail(cur, pos, msg); }

  bool eof() const { return pos >= src.size(); }
  static bool is_name_char(char c) {
    return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || (c >= '0' && c <= '9') || c == '_' || c == '-';
  }
  void skip_space(bool newlines) {
    while (!eof()) {
      const char c = src[pos];
      if (c == ' ' || c == '\t') ++pos;
      else if (c == '#') while (!eof() && src[pos] != '\n') ++pos;
      else if (newlines && (c == '\n' || c == '\r')) ++pos;
      else break;
    }
  }
  bool at_rule_start() const {   // name ::=
    size_t p = pos;
    while (p < src.size() && is_name_char(src[p])) ++p;
    if (p == pos) return false;
    while (p < src.size() && (src[p] == ' ' || src[p] == '\t')) ++p;
    return src.compare(p, 3, "::=") == 0;
  }
  std::string parse_name() {
    const size_t a = pos;
    while (!eof() && is_name_char(src[pos])) ++pos;
    if (pos == a) fail("a rule name is expected");
    return src.substr(a, pos - a);
  }
  int rule_id(const std::string& name, size_t at) {
    auto it = ids.find(name);
    if (it != ids.end()) return it->second;
    if ((int)g.rules_.size() >= kGrammarMaxRules)
      fail(cur, at, "the grammar is too large: more than " + std::to_string(kGrammarMaxRules) + " rules (groups and repeats count)");
    const int id = (int)g.rules_.size();
    g.rules_.push_back(Grammar::Rule{name, {}});
    defined.push_back(0); owner.push_back(cur); where.push_back(at);
    ids[name] = id;
    return id;
  }
  int synth_rule() {
    const std::string name = cur + "~" + std::to_string(++n_synth);   // '~' cannot appear in a user name
    const int id = rule_id(name, pos);
    defined[id] = 1;
    return id;
  }
  void charge(size_t n) {   // n more symbols
    n_elems += n;
    if (n_elems > (size_t)kGrammarMaxElems)
      fail("the grammar is too large: more than " + std::to_string(kGrammarMaxElems) + " symbols (repeats count)");
  }
  static Grammar::Elem ref_elem(int id) { Grammar::Elem e; e.ref = id; return e; }

  uint32_t hex(int n) {
    uint32_t v = 0;
    for (int i = 0; i < n; ++i, ++pos) {
      if (eof()) fail("the escape ends early");
      const char c = src[pos];
      int d = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
      if (d < 0) fail("a hexadecimal digit is expected");
      v = v * 16 + d;
    }
    if (v > 0x10FFFF) fail("the escape is not a code point");
    return v;
  }
  // one character of a literal or a class: an escape or a UTF-8 sequence of the grammar text
  uint32_t parse_char() {
    if (eof()) fail("the text ends inside a literal or a class");
    const unsigned char c = (unsigned char)src[pos];
    if (c == '\\') {
      if (pos + 1 >= src.size()) fail("the text ends inside an escape");
      const char e = src[pos + 1];
      pos += 2;
      switch (e) {
        case 'n': return '\n';
        case 'r': return '\r';
        case 't': return '\t';
        case 'x': return hex(2);
        case 'u': return hex(4);
        case 'U': return hex(8);
        case '\\': case '"': case '\'': case '[': case ']': case '-': case '^': case '.': return (unsigned char)e;
        default: pos -= 2; fail(std::string("unknown escape \\") + e);
      }
    }
    if (c == '\n' || c == '\r') fail("a line ends inside a literal or a class");
    if (c < 0x80) { ++pos; return c; }
    int n = c >= 0xF0 ? 4 : c >= 0xE0 ? 3 : c >= 0xC0 ? 2 : 0;
    if (!n || pos + n > src.size()) fail("the grammar text is not UTF-8");
    uint32_t v = c & (0xFF >> (n + 1));
    for (int i = 1; i < n; ++i) {
      const unsigned char b = (unsigned char)src[pos + i];
      if ((b & 0xC0) != 0x80) fail("the grammar text is not UTF-8");
      v = v << 6 | (b & 0x3F);
    }
    pos += n;
    return v;
  }
  int parse_int() {
    const size_t a = pos;
    long v = 0;
    while (!eof() && src[pos] >= '0' && src[pos] <= '9') {
      v = v * 10 + (src[pos++] - '0');
      if (v > 100000) fail("the repeat count is too large");
    }
    if (pos == a) fail("a number is expected");
    return (int)v;
  }

  // item{min, max} (max < 0: unbounded) appended to seq
  void repeat(std::vector<Grammar::Elem>& seq, size_t item0, int mn, int mx) {
    if (mx >= 0 && mx < mn) fail("the repeat's upper bound is below its lower bound");
    std::vector<Grammar::Elem> item(seq.begin() + item0, seq.end());
    seq.resize(item0);
    charge((size_t)mn + (mx < 0 ? 2 : 2 * (size_t)(mx - mn)));
    if (item.size() != 1) {   // several symbols (a literal): one rule for them, so a copy is one reference
      const int id = synth_rule();
      g.rules_[id].alts.push_back(item);
      item = {ref_elem(id)};
    }
    const Grammar::Elem it = item[0];
    for (int i = 0; i < mn; ++i) seq.push_back(it);
    if (mx < 0) {   // s ::= item s |
      const int s = synth_rule();
      g.rules_[s].alts.push_back({it, ref_elem(s)});
      g.rules_[s].alts.push_back({});
      seq.push_back(ref_elem(s));
    } else {        // o1 ::= item | ; ok ::= item o(k-1) |
      int prev = -1;
      for (int k = 0; k < mx - mn; ++k) {
        const int o = synth_rule();
        if (prev < 0) g.rules_[o].alts.push_back({it});
        else g.rules_[o].alts.push_back({it, ref_elem(prev)});
        g.rules_[o].alts.push_back({});
        prev = o;
      }
      if (prev >= 0) seq.push_back(ref_elem(prev));
    }
  }

  std::vector<Grammar::Elem> parse_sequence(bool nested) {
    std::vector<Grammar::Elem> seq;
    size_t item0 = 0;
    bool have_item = false;
    for (;;) {
      skip_space(true);
      if (eof()) break;
      if (!nested && at_rule_start()) break;
      const char c = src[pos];
      if (c == '|' || c == ')') break;
      if (c == '"') {
        ++pos;
        item0 = seq.size(); have_item = true;
        for (;;) {
          if (eof()) fail("the text ends inside a literal");
          if (src[pos] == '"') { ++pos; break; }
          const uint32_t cp = parse_char();
          Grammar::Elem e; e.ranges.push_back({cp, cp});
          charge(1);
          seq.push_back(e);
        }
        if (seq.size() == item0) have_item = false;   // "": nothing to repeat
      } else if (c == '[') {
        ++pos;
        Grammar::Elem e;
        if (!eof() && src[pos] == '^') { e.neg = true; ++pos; }
        for (;;) {
          if (eof()) fail("the text ends inside a class");
          if (src[pos] == ']') { ++pos; break; }
          const uint32_t a = parse_char();
          uint32_t b = a;
          if (pos + 1 < src.size() && src[pos] == '-' && src[pos + 1] != ']') {
            ++pos;
            b = parse_char();
            if (b < a) fail("the range's end is below its start");
          }
          e.ranges.push_back({a, b});
          charge(1);
        }
        merge_ranges(e.ranges);
        item0 = seq.size(); have_item = true;
        seq.push_back(e);
      } else if (c == '.') {
        ++pos;
        Grammar::Elem e; e.neg = true;
        item0 = seq.size(); have_item = true;
        charge(1);
        seq.push_back(e);
      } else if (c == '(') {
        const size_t open = pos;
        if (++depth > kGrammarMaxNesting)
          fail("groups are nested more than " + std::to_string(kGrammarMaxNesting) + " deep");
        ++pos;
        const int id = synth_rule();
        std::vector<std::vector<Grammar::Elem>> alts = parse_alternates(true);
        --depth;
        g.rules_[id].alts = std::move(alts);
        skip_space(true);
        if (eof() || src[pos] != ')') fail(cur, open, "the group is not closed");
        ++pos;
        item0 = seq.size(); have_item = true;
        charge(1);
        seq.push_back(ref_elem(id));
      } else if (is_name_char(c)) {
        const size_t at = pos;
        const std::string name = parse_name();
        item0 = seq.size(); have_item = true;
        charge(1);
        seq.push_back(ref_elem(rule_id(name, at)));
      } else if (c == '*' || c == '+' || c == '?' || c == '{') {
        if (!have_item) fail(std::string("nothing for '") + c + "' to repeat");
        int mn = 0, mx = -1;
        ++pos;
        if (c == '+') mn = 1;
        else if (c == '?') mx = 1;
        else if (c == '{') {
          skip_space(false);
          mn = parse_int();
          skip_space(false);
          if (!eof() && src[pos] == ',') {
            ++pos;
            skip_space(false);
            if (!eof() && src[pos] != '}') mx = parse_int();
            skip_space(false);
          } else {
            mx = mn;
          }
          if (eof() || src[pos] != '}') fail("'}' is expected");
          ++pos;
        }
        repeat(seq, item0, mn, mx);
        have_item = false;
      } else {
        fail(std::string("unexpected character '") + c + "'");
      }
    }
    return seq;
  }

  std::vector<std::vector<Grammar::Elem>> parse_alternates(bool nested) {
    std::vector<std::vector<Grammar::Elem>> alts;
    for (;;) {
      alts.push_back(parse_sequence(nested));
      skip_space(true);
      if (!eof() && src[pos] == '|') { ++pos; continue; }
      break;
    }
    return alts;
  }

  void run() {
    for (;;) {
      skip_space(true);
      if (eof()) break;
      const size_t at = pos;
      if (!at_rule_start()) fail("a rule (name ::= ...) is expected");
      const std::string name = parse_name();
      cur = name;
      const int id = rule_id(name, at);
      if (defined[id]) fail(name, at, "the rule is defined twice");
      defined[id] = 1; owner[id] = name; where[id] = at;
      skip_space(false);
      pos += 3;   // ::=
      std::vector<std::vector<Grammar::Elem>> alts = parse_alternates(false);
      g.rules_[id].alts = std::move(alts);
      skip_space(true);
      if (!eof() && src[pos] == ')') fail("')' without '('");
    }
    for (size_t r = 0; r < g.rules_.size(); ++r)
      if (!defined[r]) fail(owner[r], where[r], "rule \"" + g.rules_[r].name + "\" is not defined");
    auto it = ids.find("root");
    if (it == ids.end()) fail("root", src.size(), "the grammar has no rule \"root\"");
    g.root_ = it->second;
    check_left_recursion();
  }

  // Nothing here recurses: a repeat {0,n} is a chain of n rules, and a client chooses n.
  void check_left_recursion() {
    const size_t n = g.rules_.size();
    // nullable rules in one pass over the symbols: an alternative waits for `need` references, a rule
    // that turns nullable serves the alternatives it stands in
    std::vector<char> nullable(n, 0);
    struct AltRef { int rule, need; };
    std::vector<AltRef> alts;
    std::vector<std::vector<int>> used_in(n);   // rule -> indices into alts, once per occurrence
    std::vector<int> todo;
    for (size_t r = 0; r < n; ++r)
      for (const auto& alt : g.rules_[r].alts) {
        bool refs_only = true;
        for (const auto& e : alt) refs_only = refs_only && e.ref >= 0;
        if (!refs_only) continue;
        if (alt.empty()) {
          if (!nullable[r]) { nullable[r] = 1; todo.push_back((int)r); }
          continue;
        }
        for (const auto& e : alt) used_in[e.ref].push_back((int)alts.size());
        alts.push_back({(int)r, (int)alt.size()});
      }
    while (!todo.empty()) {
      const int r = todo.back();
      todo.pop_back();
      for (int a : used_in[r])
        if (--alts[a].need == 0 && !nullable[alts[a].rule]) { nullable[alts[a].rule] = 1; todo.push_back(alts[a].rule); }
    }
    std::vector<std::vector<int>> left(n);   // rules reachable at the leftmost position
    for (size_t r = 0; r < n; ++r)
      for (const auto& alt : g.rules_[r].alts)
        for (const auto& e : alt) {
          if (e.ref < 0) break;
          left[r].push_back(e.ref);
          if (!nullable[e.ref]) break;
        }
    std::vector<char> color(n, 0);               // 1: on the path, 2: done
    std::vector<std::pair<int, size_t>> path;    // (rule, next of its left[] to visit)
    for (size_t r0 = 0; r0 < n; ++r0) {
      if (color[r0]) continue;
      color[r0] = 1;
      path.push_back({(int)r0, 0});
      while (!path.empty()) {
        const int r = path.back().first;
        if (path.back().second >= left[r].size()) { color[r] = 2; path.pop_back(); continue; }
        const int t = left[r][path.back().second++];
        if (color[t] == 1) fail(owner[t], where[t], "left recursion: rule \"" + owner[t] + "\" can begin with itself");
        if (!color[t]) { color[t] = 1; path.push_back({t, 0}); }
      }
    }
  }
};

std::shared_ptr<const Grammar> Grammar::parse(const std::string& text) {
  auto g = std::shared_ptr<Grammar>(new Grammar());
  g->text_ = text;
  GrammarParser p(g->text_, *g);
  p.run();
  try {
    g->start_set();
  } catch (const std::exception& e) {   // the first state already breaks a cap: a parser error like the others
    std::string m = e.what();
    if (m.compare(0, 9, "grammar: ") == 0) m.erase(0, 9);
    p.fail("root", p.where[g->root_], m);
  }
  return g;
}

// ------------------------------------------------------------------ matcher
void Grammar::expand(Stack first, StackSet& out) const {
  std::vector<Stack> todo;   // a worklist, not recursion: the chain of leftmost references can be as long as the grammar
  todo.push_back(std::move(first));
  size_t steps = 0;
  while (!todo.empty()) {
    Stack st = std::move(todo.back());
    todo.pop_back();
    for (;;) {
      if (++steps > 64 * (size_t)kGrammarMaxStacks || out.size() > (size_t)kGrammarMaxStacks)
        throw std::runtime_error("grammar: too ambiguous: a state has more than " + std::to_string(kGrammarMaxStacks) + " stacks");
      if (st.empty()) { out.push_back(std::move(st)); break; }
      const Pos p = st.back();
      const auto& alt = rules_[p.rule].alts[p.alt];
      if ((size_t)p.idx >= alt.size()) { st.pop_back(); continue; }
      const Elem& e = alt[p.idx];
      if (e.ref < 0) { out.push_back(std::move(st)); break; }
      // a reference: go on behind it afterwards; a reference that ends its alternative leaves nothing
      // to come back to (right-recursive repeats keep a flat stack)
      if ((size_t)p.idx + 1 >= alt.size()) st.pop_back();
      else st.back().idx = p.idx + 1;
      const int n_alt = (int)rules_[e.ref].alts.size();
      for (int a = 0; a < n_alt; ++a) {
        Stack s2 = st;
        s2.push_back(Pos{e.ref, a, 0});
        todo.push_back(std::move(s2));
      }
      break;
    }
  }
}

bool Grammar::table_full() const {
  std::lock_guard<std::mutex> lk(mu_);
  return (int)sets_.size() >= kGrammarMaxSets || n_positions_ >= kGrammarMaxPositions;
}

int Grammar::intern(StackSet&& s) const {
  std::sort(s.begin(), s.end());
  s.erase(std::unique(s.begin(), s.end()), s.end());
  auto it = set_ids_.find(s);
  if (it != set_ids_.end()) return it->second;
  size_t np = 0;
  for (const Stack& st : s) np += st.size() + 1;
  if ((int)sets_.size() >= kGrammarMaxSets || n_positions_ + np > kGrammarMaxPositions)
    throw std::runtime_error("grammar: the state table is full (the text nests too deep for this grammar)");
  n_positions_ += np;
  const int id = (int)sets_.size();
  sets_.push_back(s);
  set_ids_.emplace(std::move(s), id);
  ascii_next_.resize(sets_.size() * 128, -2);
  return id;
}

int Grammar::start_set() const {
  std::lock_guard<std::mutex> lk(mu_);
  if (!sets_.empty()) return 0;
  StackSet out;
  const int n_alt = (int)rules_[root_].alts.size();
  for (int a = 0; a < n_alt; ++a) expand(Stack{Pos{root_, a, 0}}, out);
  return intern(std::move(out));
}

int Grammar::step_cp(int set, uint32_t cp) const {
  // most bytes of a vocabulary are ASCII: a flat table spares them the hash lookup
  const uint64_t key = (uint64_t)(uint32_t)set << 32 | cp;
  if (cp < 128) {
    const int32_t known = ascii_next_[(size_t)set * 128 + cp];
    if (known != -2) return known;
  } else {
    auto it = next_.find(key);
    if (it != next_.end()) return it->second;
  }
  StackSet out;
  const size_t n = sets_[set].size();
  for (size_t i = 0; i < n; ++i) {
    const Stack& st = sets_[set][i];
    if (st.empty() || !elem(st.back()).match(cp)) continue;
    Stack s2 = st;
    ++s2.back().idx;
    expand(std::move(s2), out);
  }
  const int r = out.empty() ? -1 : intern(std::move(out));
  if (cp < 128) ascii_next_[(size_t)set * 128 + cp] = r;
  else {
    if (next_.size() > (1u << 20)) next_.clear();   // a cache: it may forget
    next_.emplace(key, r);
  }
  return r;
}

// ------------------------------------------------------------------ vocabulary
GrammarVocab::GrammarVocab(const Tokenizer& tok) {
  pieces_.resize(tok.n_vocab());
  for (int i = 0; i < tok.n_vocab(); ++i) pieces_[i] = tok.piece(i);
  for (int id : {tok.eos(), tok.eot()})
    if (id >= 0 && id < tok.n_vocab() && std::find(eog_.begin(), eog_.end(), id) == eog_.end()) eog_.push_back(id);
  build();
}

GrammarVocab::GrammarVocab(std::vector<std::string> pieces, std::vector<int32_t> eog)
    : pieces_(std::move(pieces)), eog_(std::move(eog)) {
  for (int32_t id : eog_)
    if (id < 0 || id >= n_vocab()) throw std::runtime_error("grammar vocabulary: an end-of-generation id is out of range");
  build();
}

bool GrammarVocab::is_eog(int32_t id) const { return std::find(eog_.begin(), eog_.end(), id) != eog_.end(); }

void GrammarVocab::build() {
  static std::atomic<uint32_t> next_uid{1};
  uid_ = next_uid++;
  for (int i = 0; i < n_vocab(); ++i)
    if (!pieces_[i].empty() && !is_eog(i)) sorted_.push_back(i);
  std::sort(sorted_.begin(), sorted_.end(), [&](int32_t a, int32_t b) {
    const int c = pieces_[a].compare(pieces_[b]);
    return c != 0 ? c < 0 : a < b;
  });
  build_node(0, (int)sorted_.size(), 0);
}

// tokens sorted_[lo, hi) share their first `depth` bytes
int32_t GrammarVocab::build_node(int lo, int hi, int depth) {
  const int32_t me = (int32_t)nodes_.size();
  nodes_.push_back(Node{});
  int t = lo;
  while (t < hi && (int)pieces_[sorted_[t]].size() == depth) ++t;
  struct Group { uint8_t byte; int a, b; };
  std::vector<Group> groups;
  for (int a = t; a < hi;) {
    const uint8_t by = (uint8_t)pieces_[sorted_[a]][depth];
    int b = a + 1;
    while (b < hi && (uint8_t)pieces_[sorted_[b]][depth] == by) ++b;
    groups.push_back({by, a, b});
    a = b;
  }
  const int32_t e0 = (int32_t)edges_.size();
  edges_.resize(edges_.size() + groups.size());
  for (size_t k = 0; k < groups.size(); ++k) {
    const int32_t child = build_node(groups[k].a, groups[k].b, depth + 1);
    edges_[e0 + k] = Edge{groups[k].byte, child};
  }
  Node& nd = nodes_[me];
  nd.edge0 = e0; nd.n_edge = (int32_t)groups.size(); nd.tok0 = lo; nd.n_tok = t - lo;
  return me;
}

// ------------------------------------------------------------------ state
GrammarState::GrammarState(std::shared_ptr<const Grammar> g, std::shared_ptr<const GrammarVocab> v)
    : g_(std::move(g)), v_(std::move(v)) {
  if (!g_) throw std::runtime_error("grammar state: no grammar");
  cur_ = Cur{g_->start_set(), 0, 0, 0};
}

static uint32_t utf8_min(int total) { return total == 2 ? 0x80u : total == 3 ? 0x800u : 0x10000u; }

// the pending bytes can still become a character some stack accepts
bool GrammarState::pending_ok(const Cur& c) const {
  const int sh = 6 * c.remain;
  uint32_t lo = c.val << sh, hi = lo | ((1u << sh) - 1u);
  lo = std::max(lo, utf8_min(c.total));
  hi = std::min(hi, 0x10FFFFu);
  if (lo > hi) return false;
  for (const Grammar::Stack& st : g_->sets_[c.set]) {
    if (st.empty()) continue;
    const Grammar::Elem& e = g_->elem(st.back());
    // the surrogates are no characters
    if (lo < 0xD800u && e.match_any_in(lo, std::min(hi, 0xD7FFu))) return true;
    if (hi > 0xDFFFu && e.match_any_in(std::max(lo, 0xE000u), hi)) return true;
  }
  return false;
}

bool GrammarState::step_byte(Cur& c, uint8_t b) const {
  if (c.remain == 0) {
    if (b < 0x80) {
      const int ns = g_->step_cp(c.set, b);
      if (ns < 0) return false;
      c.set = ns;
      return true;
    }
    if (b >= 0xC2 && b <= 0xDF) { c.total = 2; c.val = b & 0x1F; }
    else if (b >= 0xE0 && b <= 0xEF) { c.total = 3; c.val = b & 0x0F; }
    else if (b >= 0xF0 && b <= 0xF4) { c.total = 4; c.val = b & 0x07; }
    else return false;
    c.remain = c.total - 1;
    return pending_ok(c);
  }
  if ((b & 0xC0) != 0x80) return false;
  c.val = c.val << 6 | (b & 0x3F);
  if (--c.remain > 0) return pending_ok(c);
  const uint32_t cp = c.val;
  if (cp < utf8_min(c.total) || cp > 0x10FFFF || (cp >= 0xD800 && cp <= 0xDFFF)) return false;
  const int ns = g_->step_cp(c.set, cp);
  if (ns < 0) return false;
  c = Cur{ns, 0, 0, 0};
  return true;
}

bool GrammarState::accept_text(const std::string& bytes) {
  if (!g_) throw std::runtime_error("grammar state: not initialised");
  std::lock_guard<std::mutex> lk(g_->mu_);
  Cur c = cur_;
  for (unsigned char b : bytes)
    if (!step_byte(c, b)) return false;
  cur_ = c;
  return true;
}

bool GrammarState::accept(int32_t token) {
  if (!g_ || !v_) throw std::runtime_error("grammar state: no vocabulary");
  if (token < 0 || token >= v_->n_vocab()) return false;
  if (v_->is_eog(token)) return can_end();
  const std::string& p = v_->piece(token);
  if (p.empty()) return false;
  return accept_text(p);
}

bool GrammarState::can_end() const {
  if (!g_) return false;
  std::lock_guard<std::mutex> lk(g_->mu_);
  return cur_.remain == 0 && g_->sets_[cur_.set][0].empty();   // sorted: the empty stack comes first
}

bool GrammarState::only_end() const {
  if (!g_) return false;
  std::lock_guard<std::mutex> lk(g_->mu_);
  return cur_.remain == 0 && g_->sets_[cur_.set].size() == 1 && g_->sets_[cur_.set][0].empty();
}

void GrammarState::mask(uint32_t* bits) const {
  if (!g_ || !v_) throw std::runtime_error("grammar state: no vocabulary");
  std::lock_guard<std::mutex> lk(g_->mu_);
  const size_t nw = (size_t)v_->mask_words();
  // cached per (vocabulary, state): vocabularies of several models share a grammar without evicting
  // each other, and a uid is never reused as an address can be
  const uint64_t key = (uint64_t)v_->uid() << 32 | (uint32_t)cur_.set;
  if (g_->masks_.size() > 512) g_->masks_.clear();
  if (cur_.remain == 0) {
    auto it = g_->masks_.find(key);
    if (it != g_->masks_.end()) { std::memcpy(bits, it->second.data(), nw * 4); return; }
  }
  std::memset(bits, 0, nw * 4);
  // one walk of the byte trie: the pieces that share a prefix share its steps, and a prefix no
  // stack accepts prunes every token behind it
  struct Frame { int32_t node; Cur cur; };
  std::vector<Frame> todo{{0, cur_}};
  while (!todo.empty()) {
    const Frame f = todo.back();
    todo.pop_back();
    const GrammarVocab::Node nd = v_->nodes_[f.node];
    if (f.node != 0)
      for (int k = 0; k < nd.n_tok; ++k) {
        const int32_t t = v_->sorted_[nd.tok0 + k];
        bits[t >> 5] |= 1u << (t & 31);
      }
    for (int k = 0; k < nd.n_edge; ++k) {
      const GrammarVocab::Edge& e = v_->edges_[nd.edge0 + k];
      Cur c = f.cur;
      if (step_byte(c, e.byte)) todo.push_back({e.child, c});
    }
  }
  if (cur_.remain == 0 && g_->sets_[cur_.set][0].empty())
    for (int32_t t : v_->eog_) bits[t >> 5] |= 1u << (t & 31);
  if (cur_.remain == 0) g_->masks_.emplace(key, std::vector<uint32_t>(bits, bits + nw));
}

// ------------------------------------------------------------------ JSON schema -> GBNF
namespace {

std::string gbnf_lit(const std::string& s) {
  std::string o = "\"";
  for (unsigned char c : s) {
    if (c == '\\') o += "\\\\";
    else if (c == '"') o += "\\\"";
    else if (c == '\n') o += "\\n";
    else if (c == '\r') o += "\\r";
    else if (c == '\t') o += "\\t";
    else if (c < 0x20 || c == 0x7F) { char b[8]; snprintf(b, sizeof(b), "\\x%02X", c); o += b; }
    else o += (char)c;
  }
  return o + "\"";
}

struct SchemaConv {
  const Json& root;
  std::vector<std::pair<std::string, std::string>> rules;
  std::map<std::string, std::string> refs;
  std::set<std::string> have;
  int n_obj = 0, n_any = 0, depth = 0;

  explicit SchemaConv(const Json& r) : root(r) {}

  void add(const std::string& name, const std::string& body) {
    if (have.insert(name).second) rules.push_back({name, body});
  }
  void primitives() {
    add("ws", "[ \\t\\n\\r]{0," + std::to_string(kJsonMaxSpace) + "}");
    add("char", "[^\"\\\\\\x00-\\x1F] | \"\\\\\" ( [\"\\\\/bfnrt] | \"u\" [0-9a-fA-F]{4} )");
    add("string", "\"\\\"\" char* \"\\\"\"");
    add("integer", "\"-\"? ( \"0\" | [1-9] [0-9]{0,17} )");
    add("number", "integer ( \".\" [0-9]{1,17} )? ( [eE] [-+]? [0-9]{1,3} )?");
    add("boolean", "\"true\" | \"false\"");
    add("null", "\"null\"");
  }
  void generic() {
    primitives();
    add("value", "object | array | string | number | boolean | null");
    add("member", "string ws \":\" ws value");
    add("object", "\"{\" ws ( member ( ws \",\" ws member )* )? ws \"}\"");
    add("array", "\"[\" ws ( value ( ws \",\" ws value )* )? ws \"]\"");
  }

  [[noreturn]] static void bad(const std::string& msg) { throw std::runtime_error("json schema: " + msg); }

  static bool type_ok(const Json& v, const std::string& t) {
    if (t == "object") return v.is_obj();
    if (t == "array") return v.is_arr();
    if (t == "string") return v.is_str();
    if (t == "number") return v.is_num();
    if (t == "integer") return v.is_num() && v.num() == (double)(long long)v.num();
    if (t == "boolean") return v.is_bool();
    if (t == "null") return v.is_null();
    bad("unknown type \"" + t + "\"");
  }

  const Json& resolve(const std::string& ref) const {
    for (const char* pre : {"#/$defs/", "#/definitions/"}) {
      const std::string p(pre);
      if (ref.compare(0, p.size(), p) != 0) continue;
      const std::string sec = p.substr(2, p.size() - 3), name = ref.substr(p.size());
      if (name.empty() || name.find('/') != std::string::npos) break;
      if (!root.has(sec) || !root[sec].is_obj() || !root[sec].has(name)) bad("$ref \"" + ref + "\" names nothing");
      return root[sec][name];
    }
    bad("$ref \"" + ref + "\" is not supported (only #/$defs/NAME and #/definitions/NAME)");
  }

  // the rule name of a value that fits the schema
  std::string visit(const Json& s) {
    struct Depth {   // schemas nest through $ref chains as well as through the JSON text
      int& d;
      explicit Depth(int& x) : d(x) { if (++d > 64) bad("schemas are nested more than 64 deep"); }
      ~Depth() { --d; }
    } guard(depth);
    if (s.is_bool()) {
      if (!s.boolean()) bad("the schema false allows nothing");
      generic();
      return "value";
    }
    if (!s.is_obj()) bad("a schema is an object");
    static const std::set<std::string> known = {"type", "properties", "required", "additionalProperties", "items",
                                                "minItems", "maxItems", "enum", "const", "minLength", "maxLength",
                                                "anyOf", "oneOf", "$ref", "$defs", "definitions"};
    static const std::set<std::string> notes = {"title", "description", "default", "examples", "$schema", "$id",
                                                "$comment", "deprecated", "readOnly", "writeOnly"};
    std::vector<std::string> keys;   // the constraining ones
    for (const auto& kv : s.obj()) {
      if (notes.count(kv.first)) continue;
      if (!known.count(kv.first)) bad("keyword \"" + kv.first + "\" is not supported");
      if (kv.first != "$defs" && kv.first != "definitions") keys.push_back(kv.first);
    }
    auto only = [&](const std::string& k, std::initializer_list<const char*> with) {
      for (const std::string& o : keys) {
        if (o == k) continue;
        bool ok = false;
        for (const char* w : with) ok = ok || o == w;
        if (!ok) bad("keyword \"" + o + "\" beside \"" + k + "\" is not supported");
      }
    };
    if (s.has("$ref")) {
      only("$ref", {});
      if (!s["$ref"].is_str()) bad("$ref is a string");
      const std::string ref = s["$ref"].str();
      auto it = refs.find(ref);
      if (it != refs.end()) return it->second;
      const std::string name = "ref" + std::to_string(refs.size());
      refs[ref] = name;
      const std::string target = visit(resolve(ref));
      add(name, target);
      return name;
    }
    for (const char* k : {"anyOf", "oneOf"})
      if (s.has(k)) {
        only(k, {});
        if (!s[k].is_arr() || s[k].arr().empty()) bad(std::string(k) + " is a non-empty list");
        std::string body;
        for (const Json& sub : s[k].arr()) body += (body.empty() ? "" : " | ") + visit(sub);
        const std::string name = "any" + std::to_string(n_any++);
        add(name, body);
        return name;
      }
    std::vector<std::string> types;
    if (s.has("type")) {
      if (s["type"].is_str()) types.push_back(s["type"].str());
      else if (s["type"].is_arr())
        for (const Json& t : s["type"].arr()) {
          if (!t.is_str()) bad("type is a string or a list of strings");
          types.push_back(t.str());
        }
      else bad("type is a string or a list of strings");
      if (types.empty()) bad("type is an empty list");
      for (const std::string& t : types) type_ok(Json(), t);   // throws on an unknown name
    }
    if (s.has("const") || s.has("enum")) {
      const char* k = s.has("const") ? "const" : "enum";
      only(k, {"type"});
      std::vector<Json> vals;
      if (s.has("const")) vals.push_back(s["const"]);
      else {
        if (!s["enum"].is_arr()) bad("enum is a list");
        vals = s["enum"].arr();
      }
      std::string body;
      for (const Json& v : vals) {
        bool ok = types.empty();
        for (const std::string& t : types) ok = ok || type_ok(v, t);
        if (ok) body += (body.empty() ? "" : " | ") + gbnf_lit(v.dump());
      }
      if (body.empty()) bad(std::string(k) + " allows no value of the given type");
      const std::string name = "any" + std::to_string(n_any++);
      add(name, body);
      return name;
    }
    const bool obj_keys = s.has("properties") || s.has("required") || s.has("additionalProperties");
    const bool arr_keys = s.has("items") || s.has("minItems") || s.has("maxItems");
    const bool str_keys = s.has("minLength") || s.has("maxLength");
    if (types.empty()) {
      if (obj_keys + arr_keys + str_keys > 1) bad("keywords of several types need an explicit \"type\"");
      if (obj_keys) types = {"object"};
      else if (arr_keys) types = {"array"};
      else if (str_keys) types = {"string"};
      else { generic(); return "value"; }
    }
    auto has_type = [&](const char* t) { return std::find(types.begin(), types.end(), t) != types.end(); };
    if (obj_keys && !has_type("object")) bad("object keywords beside a type that is no object");
    if (arr_keys && !has_type("array")) bad("array keywords beside a type that is no array");
    if (str_keys && !has_type("string")) bad("string keywords beside a type that is no string");
    primitives();
    std::string body;
    for (const std::string& t : types) {
      std::string r;
      if (t == "object") r = object(s);
      else if (t == "array") r = array(s);
      else if (t == "string") r = str(s);
      else r = t;
      body += (body.empty() ? "" : " | ") + r;
    }
    if (types.size() == 1) return body;
    const std::string name = "any" + std::to_string(n_any++);
    add(name, body);
    return name;
  }

  static int count(const Json& s, const char* k, int dflt) {
    if (!s.has(k)) return dflt;
    if (!s[k].is_num() || s[k].num() < 0 || s[k].num() != (double)(int)s[k].num() || s[k].num() > 10000)
      bad(std::string(k) + " is a whole number from 0 to 10000");
    return (int)s[k].num();
  }

  std::string str(const Json& s) {
    if (!s.has("minLength") && !s.has("maxLength")) return "string";
    const int mn = count(s, "minLength", 0), mx = count(s, "maxLength", -1);
    if (mx >= 0 && mx < mn) bad("maxLength is below minLength");
    const std::string name = "any" + std::to_string(n_any++);
    add(name, "\"\\\"\" char{" + std::to_string(mn) + "," + (mx < 0 ? "" : std::to_string(mx)) + "} \"\\\"\"");
    return name;
  }

  std::string array(const Json& s) {
    std::string item = "value";
    if (s.has("items")) {
      if (s["items"].is_arr()) bad("keyword \"items\" as a list (tuple form) is not supported");
      item = visit(s["items"]);
    } else {
      generic();
    }
    const int mn = count(s, "minItems", 0), mx = count(s, "maxItems", -1);
    if (mx >= 0 && mx < mn) bad("maxItems is below minItems");
    const std::string name = "any" + std::to_string(n_any++);
    std::string body;
    if (mx == 0) body = "\"[\" ws \"]\"";
    else {
      const std::string more = "( ws \",\" ws " + item + " ){" + std::to_string(std::max(mn - 1, 0)) + "," +
                               (mx < 0 ? "" : std::to_string(mx - 1)) + "}";
      body = mn > 0 ? "\"[\" ws " + item + " " + more + " ws \"]\"" : "\"[\" ws ( " + item + " " + more + " )? ws \"]\"";
    }
    add(name, body);
    return name;
  }

  // the contents of a key string that is none of `keys` (plain characters only, no escapes)
  std::string not_keys(const std::string& base, const std::vector<std::string>& keys) {
    add("plain", "[^\"\\\\\\x00-\\x1F]");
    int n = 0;
    std::function<std::string(const std::string&)> node = [&](const std::string& prefix) {
      const std::string name = base + "-n" + std::to_string(n++);
      std::set<unsigned char> next;
      bool terminal = false;
      for (const std::string& k : keys) {
        if (k.compare(0, prefix.size(), prefix) != 0) continue;
        if (k.size() == prefix.size()) terminal = true;
        else next.insert((unsigned char)k[prefix.size()]);
      }
      std::string body, cls = "[^\"\\\\\\x00-\\x1F";
      for (unsigned char c : next) {
        char b[8];
        snprintf(b, sizeof(b), "\\x%02X", c);
        cls += b;
        body += (body.empty() ? "" : " | ") + (std::string("\"") + b + "\" ") + node(prefix + (char)c);
      }
      body += (body.empty() ? "" : " | ") + cls + "] plain*";
      if (!terminal) body += " | ";
      add(name, body);
      return name;
    };
    return node("");
  }

  std::string object(const Json& s) {
    const std::string base = "o" + std::to_string(n_obj++);
    std::vector<std::string> keys;
    std::vector<std::string> vals;
    if (s.has("properties")) {
      if (!s["properties"].is_obj()) bad("properties is an object");
      for (const auto& kv : s["properties"].obj()) { keys.push_back(kv.first); vals.push_back(visit(kv.second)); }
    }
    bool addl = false;
    std::string addl_val = "value";
    if (s.has("additionalProperties")) {
      const Json& a = s["additionalProperties"];
      if (a.is_bool()) addl = a.boolean();
      else { addl = true; addl_val = visit(a); }
      if (addl && addl_val == "value") generic();
    }
    std::set<std::string> required;
    if (s.has("required")) {
      if (!s["required"].is_arr()) bad("required is a list of names");
      for (const Json& r : s["required"].arr()) {
        if (!r.is_str()) bad("required is a list of names");
        required.insert(r.str());
        if (std::find(keys.begin(), keys.end(), r.str()) == keys.end())
          bad("required key \"" + r.str() + "\" is not in properties");
      }
    }
    const size_t k = keys.size();
    for (size_t i = 0; i < k; ++i)
      add(base + "-k" + std::to_string(i), gbnf_lit(Json(keys[i]).dump()) + " ws \":\" ws " + vals[i]);
    if (addl) {
      std::string akey = "string";
      if (k) {
        for (const std::string& key : keys) {
          if (key.size() > 256) bad("additionalProperties beside a property name longer than 256 bytes is not supported");
          for (unsigned char c : key)
            if (c < 0x20 || c >= 0x7F || c == '"' || c == '\\')
              bad("additionalProperties beside the property name \"" + key + "\" (only printable ASCII names without quote and backslash are supported there)");
        }
        akey = "\"\\\"\" " + not_keys(base, keys) + " \"\\\"\"";
      }
      add(base + "-a", akey + " ws \":\" ws " + addl_val);
    }
    // r<i>-f / r<i>-n: the members from property i on, before / after the object's first member
    for (size_t i = k + 1; i-- > 0;)
      for (int first = 0; first < 2; ++first) {
        const std::string sep = first ? "" : "ws \",\" ws ";
        auto rname = [&](size_t j, int f) { return base + "-r" + std::to_string(j) + (f ? "-f" : "-n"); };
        std::string body;
        if (addl) body = sep + base + "-a " + rname(i, 0);
        if (i < k) {
          body += (body.empty() ? "" : " | ") + sep + base + "-k" + std::to_string(i) + " " + rname(i + 1, 0);
          if (!required.count(keys[i])) body += " | " + rname(i + 1, first);
        } else {
          body += body.empty() ? "" : " | ";   // the empty alternative: the object ends
        }
        add(rname(i, first), body);
      }
    add(base, "\"{\" ws " + base + "-r0-f ws \"}\"");
    return base;
  }
};

}  // namespace

std::string json_schema_to_gbnf(const Json& schema) {
  SchemaConv c(schema);
  std::string root;
  if (schema.is_obj() && schema.get_str("type", "") == "json_object") {
    for (const auto& kv : schema.obj())
      if (kv.first != "type") SchemaConv::bad("keyword \"" + kv.first + "\" beside the type json_object is not supported");
    c.generic();
    root = "object";
  } else {
    root = c.visit(schema);
  }
  std::string out = "root ::= " + root + "\n";
  for (const auto& r : c.rules) out += r.first + " ::= " + r.second + "\n";
  return out;
}

}  // namespace mp
