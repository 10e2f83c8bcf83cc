"""Grammar-constrained generation, host side (csrc/runtime/grammar.cpp): GBNF grammars and JSON
schemas turned into per-state token masks for `Engine.set_slot_masks`.

    g = Grammar(gbnf='root ::= "yes" | "no"', tokenizer=tok)       # or json_schema={...}
    st = g.state()
    eng.set_slot_masks([0], [st.mask()])       # before start() / admit(): the first token is constrained
    ... after each round:  st.accept(token); eng.set_slot_masks([0], [st.mask()])

GBNF subset: rules `name ::= ...` (`root` required), sequences, `|`, groups, `* + ? {m} {m,} {m,n}`,
literals with the escapes \\n \\r \\t \\\\ \\" \\xHH \\uHHHH \\UHHHHHHHH, classes `[a-z]`, `[^...]`, `.`,
`#` comments.  Matching is over Unicode code points; a token that ends inside a character is
allowed when some completion of the character is.  Control tokens and tokens with an empty piece
are never allowed; the end-of-generation tokens exactly when the text may end (`can_end`).
"""
from __future__ import annotations

import ctypes
import json

import numpy as np

from . import _native as N


def json_schema_to_gbnf(schema) -> str:
    """The GBNF grammar of the JSON documents that fit `schema` (a dict or a JSON string).
    {"type": "json_object"} gives any JSON object.  Raises naming an unsupported keyword."""
    text = schema if isinstance(schema, str) else json.dumps(schema)
    r = N.lib().mp_json_schema_to_gbnf(N.cstr(text))
    if r is None:
        N.check(None, "json_schema_to_gbnf")
    return r.decode("utf-8")


class Grammar:
    def __init__(self, gbnf: str | None = None, json_schema=None, tokenizer=None):
        if (gbnf is None) == (json_schema is None):
            raise ValueError("Grammar: give exactly one of gbnf and json_schema")
        self.gbnf = gbnf if gbnf is not None else json_schema_to_gbnf(json_schema)
        self.tokenizer = tokenizer   # keeps the native tokenizer alive while the vocabulary is built
        h = N.lib().mp_grammar_parse(N.cstr(self.gbnf), tokenizer._h if tokenizer is not None else None)
        if not h:
            N.check(None, "grammar")
        self._h = ctypes.c_void_p(h)

    def state(self) -> "State":
        s = N.lib().mp_grammar_state_new(self._h)
        if not s:
            N.check(None, "grammar state")
        return State(self, ctypes.c_void_p(s))

    def close(self):
        if getattr(self, "_h", None):
            N.lib().mp_grammar_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class State:
    """Where a text stands in a grammar.  accept / accept_text return False and leave the state
    unchanged when the token or the bytes cannot follow."""

    def __init__(self, grammar: Grammar, handle):
        self.grammar = grammar
        self._s = handle

    def clone(self) -> "State":
        s = N.lib().mp_grammar_state_clone(self._s)
        if not s:
            N.check(None, "grammar state clone")
        return State(self.grammar, ctypes.c_void_p(s))

    def accept(self, token: int) -> bool:
        return bool(N.check(N.lib().mp_grammar_accept(self._s, int(token)), "grammar accept"))

    def accept_text(self, data) -> bool:
        b = data.encode("utf-8") if isinstance(data, str) else bytes(data)
        return bool(N.check(N.lib().mp_grammar_accept_text(self._s, b, len(b)), "grammar accept_text"))

    def mask(self, n_vocab: int | None = None) -> np.ndarray:
        """uint32 words, bit t of word t >> 5 set iff token t is allowed.  n_vocab: the engine's
        vocabulary size when it is padded past the tokenizer's (the extra ids stay banned)."""
        nw = N.check(N.lib().mp_grammar_mask_words(self._s), "grammar mask")
        if n_vocab is not None:
            nw = max(nw, (int(n_vocab) + 31) // 32)
        bits = np.zeros(nw, np.uint32)
        N.check(N.lib().mp_grammar_mask(self._s, bits.ctypes.data, nw), "grammar mask")
        return bits

    @property
    def can_end(self) -> bool:
        return bool(N.check(N.lib().mp_grammar_can_end(self._s), "grammar can_end"))

    @property
    def only_end(self) -> bool:
        return bool(N.check(N.lib().mp_grammar_only_end(self._s), "grammar only_end"))

    def __del__(self):
        try:
            if getattr(self, "_s", None):
                N.lib().mp_grammar_state_free(self._s)
                self._s = None
        except Exception:
            pass
