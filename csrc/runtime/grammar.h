// Grammar-constrained generation, host side: a GBNF parser, a pushdown matcher over Unicode code
// points, per-state token masks over a tokenizer's vocabulary, and a JSON-schema -> GBNF converter.
// The masks feed Engine::set_slot_masks (row_mask.hip bans every other token on the device).
//
// GBNF subset (the public notation of llama.cpp's grammars):
//   name ::= ...            rules; "root" is required; a rule runs until the next `name ::=`
//   a b | c   ( ... )       sequences, alternatives, groups
//   x* x+ x? x{m} x{m,} x{m,n}
//   "lit"                   escapes \n \r \t \\ \" \' \[ \] \xHH \uHHHH \UHHHHHHHH
//   [a-z0-9_] [^...] .      character classes (same escapes), negated classes, any character
//   # comment
// Errors (std::runtime_error) name the rule and the line:column: syntax, undefined rule, missing
// root, left recursion.  Token literals, lazy grammars and trigger words are not supported.
#pragma once
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "json.h"

namespace mp {

class Tokenizer;

// Grammars come from clients: every size is capped and nothing recurses on the grammar's depth, so a
// hostile text ends in a parser error (or, while matching, in a std::runtime_error), never in a crash.
constexpr int kGrammarMaxRules = 32768;        // rules, the synthesized ones of groups and repeats included
constexpr int kGrammarMaxElems = 262144;       // symbols over all rules
constexpr int kGrammarMaxNesting = 128;        // groups inside groups
constexpr int kGrammarMaxStacks = 65536;       // stacks of one state (an ambiguous grammar multiplies them)
constexpr int kGrammarMaxSets = 65536;         // interned states of one parsed grammar ...
constexpr size_t kGrammarMaxPositions = 1u << 20;   // ... and the stack entries they hold together

class Grammar {
 public:
  static std::shared_ptr<const Grammar> parse(const std::string& text);
  const std::string& text() const { return text_; }
  // the state tables are full (kGrammarMaxSets / kGrammarMaxPositions): matching throws from here on.
  // States hold ids into the tables, so they are never evicted; parse the text again for fresh ones.
  bool table_full() const;

  struct Elem {                 // one symbol of an alternative
    int ref = -1;               // >= 0: rule reference; otherwise a character set
    bool neg = false;           // [^...]
    std::vector<std::pair<uint32_t, uint32_t>> ranges;   // sorted, inclusive ("." is [^] = neg with no ranges)
    bool match(uint32_t cp) const;
    bool match_any_in(uint32_t lo, uint32_t hi) const;   // some code point of [lo, hi] matches
  };
  struct Rule {
    std::string name;
    std::vector<std::vector<Elem>> alts;
  };
  // a position inside the grammar, and a pushdown stack of them: the back is the character set to
  // match next, the entries below are where to go on when the rule above is finished
  struct Pos {
    int32_t rule, alt, idx;
    bool operator==(const Pos& o) const { return rule == o.rule && alt == o.alt && idx == o.idx; }
    bool operator<(const Pos& o) const {
      return rule != o.rule ? rule < o.rule : alt != o.alt ? alt < o.alt : idx < o.idx;
    }
  };
  using Stack = std::vector<Pos>;
  using StackSet = std::vector<Stack>;   // sorted, distinct; an empty Stack = the grammar may end here

 private:
  friend class GrammarState;
  friend struct GrammarParser;
  std::string text_;
  std::vector<Rule> rules_;
  int root_ = -1;

  const Elem& elem(const Pos& p) const { return rules_[p.rule].alts[p.alt][p.idx]; }
  void expand(Stack st, StackSet& out) const;   // st -> the stacks whose back is a character set
  // Stack sets are interned: a GrammarState holds an id.  Transitions and masks are cached per id.
  // The tables only grow (with the depth of the nesting a text reaches); one mutex guards them.
  mutable std::mutex mu_;
  mutable std::vector<StackSet> sets_;
  mutable std::map<StackSet, int> set_ids_;
  mutable std::unordered_map<uint64_t, int> next_;              // (set << 32 | cp) -> set, -1 = dead
  mutable std::vector<int32_t> ascii_next_;                     // the same for cp < 128: [set * 128 + cp], -2 = not known yet
  mutable std::unordered_map<uint64_t, std::vector<uint32_t>> masks_;   // (vocabulary uid << 32 | set), no pending bytes
  mutable size_t n_positions_ = 0;
  int intern(StackSet&& s) const;
  int step_cp(int set, uint32_t cp) const;   // -1: no stack accepts cp
  int start_set() const;
};

// Every token's bytes (Tokenizer::piece) as a byte trie, and the end-of-generation ids.  Control
// tokens and tokens with an empty piece are never allowed; EOG exactly when the grammar may end.
class GrammarVocab {
 public:
  explicit GrammarVocab(const Tokenizer& tok);
  GrammarVocab(std::vector<std::string> pieces, std::vector<int32_t> eog);
  int n_vocab() const { return (int)pieces_.size(); }
  int mask_words() const { return (n_vocab() + 31) / 32; }
  const std::string& piece(int32_t id) const { return pieces_[id]; }
  bool is_eog(int32_t id) const;
  uint32_t uid() const { return uid_; }   // distinct for every vocabulary object of the process (mask cache key)

 private:
  friend class GrammarState;
  struct Node { int32_t edge0 = 0, n_edge = 0, tok0 = 0, n_tok = 0; };
  struct Edge { uint8_t byte; int32_t child; };
  void build();
  int32_t build_node(int lo, int hi, int depth);
  uint32_t uid_ = 0;
  std::vector<std::string> pieces_;
  std::vector<int32_t> eog_;
  std::vector<int32_t> sorted_;   // token ids by piece (the trie's token lists index into it)
  std::vector<Node> nodes_;
  std::vector<Edge> edges_;
};

// Where a text stands in a grammar: the stack set and the bytes of an unfinished UTF-8 sequence.
class GrammarState {
 public:
  GrammarState() = default;
  GrammarState(std::shared_ptr<const Grammar> g, std::shared_ptr<const GrammarVocab> v);
  // true: the token (its bytes; EOG: the end) is allowed here and the state moved; false: unchanged
  bool accept(int32_t token);
  bool accept_text(const std::string& bytes);
  // bits: mask_words() words; bit t set iff token t is allowed (the grammar can consume all its bytes;
  // a token that ends inside a character: some completion of the character is acceptable)
  void mask(uint32_t* bits) const;
  bool can_end() const;    // the text so far is a whole sentence
  bool only_end() const;   // ... and nothing can follow it
  bool valid() const { return g_ != nullptr; }
  const std::shared_ptr<const GrammarVocab>& vocab() const { return v_; }

 private:
  struct Cur { int set; uint32_t val; int8_t remain, total; };
  bool step_byte(Cur& c, uint8_t b) const;   // caller holds g_->mu_
  bool pending_ok(const Cur& c) const;
  std::shared_ptr<const Grammar> g_;
  std::shared_ptr<const GrammarVocab> v_;
  Cur cur_{0, 0, 0, 0};
};

// JSON schema -> GBNF.  Supported: type (string or list: object, array, string, number, integer,
// boolean, null), properties / required / additionalProperties (false by default), items / minItems /
// maxItems, enum, const, minLength / maxLength, anyOf / oneOf, local $ref into #/$defs and
// #/definitions; {"type": "json_object"} is any JSON object.  Any other constraining keyword throws
// naming it.  Properties come out in the order Json holds them: sorted by key (std::map).  Optional
// whitespace between JSON tokens is at most kJsonMaxSpace characters.
constexpr int kJsonMaxSpace = 16;
std::string json_schema_to_gbnf(const Json& schema);

}  // namespace mp
