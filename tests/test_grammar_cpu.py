"""The host grammar engine (csrc/runtime/grammar.cpp) through mipipe.grammar, with the tiny-l3
vocabulary (trained byte-level BPE, 4096 entries): the GBNF parser, the matcher against languages the
test enumerates itself, every token's mask bit against a byte-prefix oracle, and random token walks."""
import itertools
import random

import numpy as np
import pytest

from conftest import make_model

# ---------------------------------------------------------------- finite languages, enumerated here
def _cat(*parts):
    return {"".join(p) for p in itertools.product(*parts)}


def _rep(alts, lo, hi):
    out = set()
    for k in range(lo, hi + 1):
        out |= {"".join(p) for p in itertools.product(alts, repeat=k)}
    return out


LANGS = {
    "colours": ('root ::= ("red" | "green" | "blue") " " pet{1,2} [0-3] ("!" | "?")?\npet ::= "cat" | "dog"\n',
                _cat(["red", "green", "blue"], [" "], _rep(["cat", "dog"], 1, 2), "0123", ["", "!", "?"])),
    "codes": ('root ::= [a-c]{2} "-" ([0-4] | "x"){1,2}',
              _cat(_rep("abc", 2, 2), ["-"], _rep("01234x", 1, 2))),
    "unicode": ('root ::= ("é" | "日本" | "ñu" | "\\U0001F642") ("語" | "l")? [α-γ]{1,2} ("ok" | "да")',
                _cat(["é", "日本", "ñu", "\U0001F642"], ["", "語", "l"], _rep("αβγ", 1, 2), ["ok", "да"])),
    "pairs": ('root ::= [a-z]{2} ("!" | "?")?',
              _cat(_rep("abcdefghijklmnopqrstuvwxyz", 2, 2), ["", "!", "?"])),
}
assert [len(m) for _, m in LANGS.values()] == [216, 378, 288, 2028]


def _byte_prefixes(members):
    out = set()
    for m in members:
        b = m.encode()
        out.update(b[:k] for k in range(len(b) + 1))
    return out


@pytest.fixture(scope="module")
def tok(native, model_dir):
    from mipipe.tokenizer import Tokenizer
    path, cfg = make_model(model_dir, "tiny-l3", "Q8_0")
    t = Tokenizer(path)
    assert t.n_vocab == 4096
    return t


@pytest.fixture(scope="module")
def pieces(tok):
    return [tok.piece(i) for i in range(tok.n_vocab)]


@pytest.fixture(scope="module")
def langs(tok):
    """name -> (Grammar with the vocabulary, members as bytes, every byte prefix of a member)"""
    from mipipe.grammar import Grammar
    out = {}
    for name, (gbnf, members) in LANGS.items():
        mb = {m.encode() for m in members}
        out[name] = (Grammar(gbnf=gbnf, tokenizer=tok), mb, _byte_prefixes(members))
    return out


# ---------------------------------------------------------------- parser
CONSTRUCTS = [
    ('root ::= "a" "b"', ["ab"], ["a", "abc", "ba"]),
    ('root ::= "a" | "b" | ', ["a", "b", ""], ["ab"]),
    ('root ::= ("a" | "b") "c"', ["ac", "bc"], ["c", "abc"]),
    ('root ::= "a"* "b"', ["b", "aaab"], ["a", "ba"]),
    ('root ::= "ab"+', ["ab", "abab"], ["", "aba"]),
    ('root ::= "a"? "b"', ["b", "ab"], ["aab"]),
    ('root ::= "a"{2}', ["aa"], ["a", "aaa"]),
    ('root ::= "a"{2,}', ["aa", "aaaaa"], ["a"]),
    ('root ::= "a"{1,3}', ["a", "aaa"], ["", "aaaa"]),
    ('root ::= "\\n\\r\\t\\\\\\"\\x41\\u00e9\\U0001F642"', ['\n\r\t\\"Aé\U0001F642'], ["nrt"]),
    ('root ::= [a-z0-9_]+', ["a_9"], ["A", ""]),
    ('root ::= [^a-z\\n]', ["A", "é", "\U0001F642"], ["a", "\n", "AA"]),
    ('root ::= [\\x41-\\u00e9]', ["A", "é", "a"], ["ê", "@"]),
    ('root ::= . "."', ["x.", "日."], [".", "xy"]),
    ('# a comment\nroot ::= item  # another\n  ("," item)*\n\nitem ::= [0-9]\n', ["1", "1,2,3"], ["1,", ",1"]),
    ('root ::= a\na ::= "(" a ")" | "x"', ["x", "((x))"], ["(x", "()"]),
]


@pytest.mark.parametrize("gbnf,yes,no", CONSTRUCTS)
def test_constructs_parse_and_match(native, gbnf, yes, no):
    from mipipe.grammar import Grammar
    g = Grammar(gbnf=gbnf)
    for s in yes:
        st = g.state()
        assert st.accept_text(s) and st.can_end, (gbnf, s)
    for s in no:
        st = g.state()
        assert not (st.accept_text(s) and st.can_end), (gbnf, s)


ERRORS = [
    ('root ::= "a" ]', "root", "unexpected"),                     # syntax
    ('root ::= thing\nthing ::= ("a" | "b"', "thing", "not closed"),
    ('root ::= "a\nb"', "root", "line ends"),
    ('root ::= "a"{3,2}', "root", "bound"),
    ('root ::= item\nitem ::= "a" other', "item", '"other" is not defined'),   # undefined rule
    ('start ::= "a"', "root", 'no rule "root"'),                   # missing root
    ('root ::= expr\nexpr ::= expr "+" "1" | "1"', "expr", "left recursion"),
    ('root ::= a\na ::= b "x"\nb ::= a | "y"', "a", "left recursion"),
    ('root ::= a\na ::= opt a "x" | "y"\nopt ::= "o"?', "a", "left recursion"),   # through a nullable prefix
]


@pytest.mark.parametrize("gbnf,rule,what", ERRORS)
def test_errors_name_rule_and_position(native, gbnf, rule, what):
    from mipipe.grammar import Grammar
    with pytest.raises(RuntimeError) as e:
        Grammar(gbnf=gbnf)
    msg = str(e.value)
    assert f'rule "{rule}"' in msg and what in msg and "line " in msg and "column " in msg, msg


# Grammars come from clients (the server's `grammar` field): sizes are capped and nothing recurses on the
# grammar's depth, so a hostile text is a parser error that names the rule, not a crash of the process.
HOSTILE = [
    ("repeat_count", 'root ::= ("a"?){0,100000}', "root", "too large"),
    ("open_groups", "root ::= " + "(" * 60000 + '"a"' + ")" * 60000, "root", "nested more than"),
    ("long_literal", 'root ::= "' + "x" * 300000 + '"', "root", "too large"),
    ("many_rules", "root ::= r0\n" + "".join(f"r{i} ::= r{i + 1}\n" for i in range(40000)) + 'r40000 ::= "a"\n', "r", "too large"),
    ("ambiguous", "root ::=" + " n" * 40 + '\nn ::= | "a" | ', "root", "too ambiguous"),
]


@pytest.mark.parametrize("name,gbnf,rule,what", HOSTILE, ids=[h[0] for h in HOSTILE])
def test_hostile_grammars_are_parser_errors(native, name, gbnf, rule, what):
    from mipipe.grammar import Grammar
    with pytest.raises(RuntimeError) as e:
        Grammar(gbnf=gbnf)
    msg = str(e.value)
    assert f'rule "{rule}' in msg and what in msg and "line " in msg, msg[:300]


def test_long_chains_parse_and_match_without_recursion(native):
    """Just under the caps: a repeat chain and a chain of rules 30000 long parse, match and end."""
    from mipipe.grammar import Grammar
    st = Grammar(gbnf='root ::= "a"{0,30000} "b"').state()
    assert st.accept_text("a" * 2000 + "b") and st.can_end and st.only_end
    chain = "root ::= r0\n" + "".join(f"r{i} ::= r{i + 1} | \n" for i in reversed(range(30000))) + 'r30000 ::= "a"?\n'
    st = Grammar(gbnf=chain).state()
    assert st.can_end and st.accept_text("a") and st.only_end and not st.clone().accept_text("a")


def test_deep_nesting_ends_in_an_error_not_a_crash(native):
    """A recursive grammar's state table is bounded: the text that nests past it gets an error."""
    from mipipe.grammar import Grammar
    st = Grammar(gbnf='root ::= "(" root ")" "x" | "a"').state()
    assert st.accept_text("(" * 100)
    with pytest.raises(RuntimeError, match="state table is full"):
        for _ in range(1 << 16):
            assert st.accept_text("(" * 64)
    assert not st.can_end                            # the failed call left the state where it was
    again = Grammar(gbnf='root ::= "(" root ")" "x" | "a"').state()       # a fresh parse has fresh tables
    assert again.accept_text("((a)x)x") and again.only_end


# ---------------------------------------------------------------- finite-language oracle
@pytest.mark.parametrize("name", list(LANGS))
def test_accept_text_matches_enumeration(langs, name):
    g, members, prefixes = langs[name]
    rng = random.Random(name)
    strs = sorted(LANGS[name][1])
    alphabet = sorted({c for m in strs for c in m}) + ["z", "9", " ", "語"]
    cands = set()
    for m in rng.sample(strs, 60):
        cands.update(m[:k] for k in range(len(m) + 1))
        for _ in range(4):                                  # one character replaced, inserted or dropped
            k = rng.randrange(len(m) + 1)
            cands.add(m[:k] + rng.choice(alphabet) + m[k + rng.randrange(2):])
            cands.add(m + rng.choice(alphabet))
    n_yes = n_member = 0
    for s in sorted(cands):
        b = s.encode()
        st = g.state()
        ok = st.accept_text(s)
        assert ok == (b in prefixes), (name, s)
        if ok:
            n_yes += 1
            assert st.can_end == (b in members), (name, s)
            n_member += b in members
        else:
            assert not st.can_end                           # unchanged: still at the start
    assert n_yes > 100 and n_member >= 60 and len(cands) - n_yes > 50


def test_bytes_inside_a_character(langs):
    g, members, prefixes = langs["unicode"]
    st = g.state()
    assert st.accept_text("日本".encode()[:4]) and not st.can_end      # one character and a third
    assert not st.clone().accept_text(b"\x80\x80")                      # U+6000 is a character, but not the one that follows
    assert st.accept_text("日本".encode()[4:] + "α".encode()[:1])
    assert not st.clone().accept_text(b"\x20")                          # a character may not stop half way
    assert st.accept_text("α".encode()[1:] + b"ok") and st.can_end and st.only_end
    assert not g.state().accept_text(b"\xc3\x28") and not g.state().accept_text(b"\xff")


# ---------------------------------------------------------------- masks
def _states(langs, per_lang=9):
    """(name, prefix bytes, state) reached by byte prefixes of members, the start included."""
    out = []
    for name, (g, members, prefixes) in langs.items():
        rng = random.Random("mask" + name)
        picks = [b""] + rng.sample(sorted(p for p in prefixes if p and p not in members), per_lang - 3)
        picks += rng.sample(sorted(members), 2)
        for p in picks:
            st = g.state()
            assert st.accept_text(p), (name, p)
            out.append((name, p, st))
    return out


def test_every_token_bit_against_the_oracle(langs, tok, pieces):
    states = _states(langs)
    assert len(states) >= 30
    eog = {t for t in (tok.eos, tok.eot) if t >= 0}
    assert eog and all(pieces[t] == b"" for t in eog)
    empty = [i for i, p in enumerate(pieces) if not p]
    assert len(empty) > 256                                  # control and filler tokens
    ids = np.arange(tok.n_vocab)
    masks, counts, partial = [], [], 0
    for name, prefix, st in states:
        bits = st.mask()
        assert bits.dtype == np.uint32 and bits.size == (tok.n_vocab + 31) // 32
        got = ((bits[ids >> 5] >> (ids & 31).astype(np.uint32)) & 1).astype(bool)
        masks.append(got)
        counts.append(int(got.sum()))
    # not vacuous, asserted before the comparison: every state allows something, one allows a lot
    assert min(counts) >= 1 and max(counts) > 100, counts
    for (name, prefix, st), got in zip(states, masks):
        _, members, prefixes = langs[name]
        want = np.array([bool(p) and (prefix + p) in prefixes for p in pieces])
        for t in eog:
            want[t] = st.can_end
        assert st.can_end == (prefix in members)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (name, prefix, [(int(t), pieces[t], bool(got[t])) for t in bad[:6]])
        assert not got[[t for t in empty if t not in eog]].any()
        for t in np.flatnonzero(got):
            if pieces[t]:
                try:
                    (prefix + pieces[t]).decode()
                except UnicodeDecodeError:
                    partial += 1
    assert partial > 0, "no allowed token ends inside a character: the non-ASCII grammar tests nothing"


def test_mask_is_the_same_for_a_cloned_and_a_revisited_state(langs):
    g, members, _ = langs["colours"]
    a = g.state()
    assert a.accept_text("red cat")
    b = a.clone()
    first = a.mask()
    assert np.array_equal(first, b.mask()) and np.array_equal(first, a.mask())
    assert b.accept_text("dog") and not np.array_equal(b.mask(), first)
    assert np.array_equal(a.mask(), first)                   # the clone moved, the original did not


# ---------------------------------------------------------------- token paths
def test_random_token_walks(langs, tok, pieces):
    rng = random.Random(2024)
    eog = {t for t in (tok.eos, tok.eot) if t >= 0}
    names = list(langs)
    ended = stopped_on_eog = 0
    for w in range(200):
        g, members, prefixes = langs[names[w % len(names)]]
        st, text = g.state(), b""
        for _ in range(64):
            bits = st.mask()
            allowed = np.flatnonzero(np.unpackbits(bits.view(np.uint8), bitorder="little")[:tok.n_vocab])
            assert allowed.size
            t = int(rng.choice(allowed))
            if t in eog:
                assert st.can_end and st.accept(t) and text in members
                stopped_on_eog += 1
                break
            assert st.accept(t), (text, t)
            text += pieces[t]
            assert text in prefixes, text
            if st.only_end:
                assert text in members
                ended += 1
                break
        else:
            raise AssertionError("a walk in a finite language did not end")
    assert ended > 100 and ended + stopped_on_eog == 200


# ---------------------------------------------------------------- the engine's mask life cycle (CPU backend)
def test_masks_through_start_survive_a_second_generation(native, model_dir, tok):
    """Two generations on one engine without a release(): masks passed to start() constrain both; a mask
    left over from the first generation does not leak into a start() without masks."""
    from mipipe.engine import Engine
    from mipipe.grammar import Grammar
    path, cfg = make_model(model_dir, "tiny-l3", "Q8_0")
    g = Grammar(gbnf='root ::= ("yes" | "no") "!"', tokenizer=tok)
    members = {b"yes!", b"no!"}
    ps = [[1, 5, 9], [1, 7]]

    def generate(eng, st):
        text = b""
        for _ in range(8):
            t = eng.tokens()[0][-1]
            assert st.accept(t), (text, t)
            text += tok.piece(t)
            if st.only_end:
                return text
            eng.set_slot_masks([0], [st.mask(cfg.vocab)])
            eng.decode(1)
        raise AssertionError(text)

    with Engine(gguf=path, backend="cpu", max_ctx=128, n_mb=1, mb_size=2, threads=2) as eng:
        eng.start(ps)
        eng.decode(3)
        free = eng.tokens()
    with Engine(gguf=path, backend="cpu", max_ctx=128, n_mb=1, mb_size=2, threads=2, row_masks=True) as eng:
        for _ in range(2):                                   # the second time slot 0 is still busy with the first
            st = g.state()
            eng.start(ps, masks=[st.mask(cfg.vocab), None])
            assert generate(eng, st) in members
        eng.start(ps)                                        # the mask the second generation left is gone
        eng.decode(3)
        assert eng.tokens() == free
        with pytest.raises(RuntimeError, match="listed twice"):
            eng.set_slot_masks([1, 1], [st.mask(cfg.vocab), None])
        with pytest.raises(ValueError):
            eng.start(ps, masks=[None])
