"""json_schema_to_gbnf (csrc/runtime/grammar.cpp) through mipipe.grammar: for every supported keyword,
hand-listed instances that fit the schema are accepted whole (compact json.dumps with sorted keys: the
converter emits properties in key order) and hand-listed instances that do not are rejected."""
import json

import pytest

NODE = {"type": "object", "properties": {"v": {"type": "integer"}, "next": {"$ref": "#/$defs/node"}}, "required": ["v"]}

# (name, schema, valid instances, invalid instances)
CASES = [
    ("required_and_enum",
     {"type": "object", "properties": {"age": {"type": "integer"}, "kind": {"enum": ["a", "b"]}, "note": {"type": "string"}},
      "required": ["age", "kind"]},
     [{"age": 3, "kind": "a"}, {"age": -40, "kind": "b", "note": "hé \"x\"\n"}, {"age": 0, "kind": "a", "note": ""}],
     [{"kind": "a"},                                  # a required key is missing
      {"age": 3, "kind": "a", "zzz": 1},              # an extra key
      {"age": "3", "kind": "a"}, {"age": 3.5, "kind": "a"},   # wrong types
      {"age": 3, "kind": "c"},                        # outside the enum
      {"age": 3, "kind": "a", "note": 7}, [], "x"]),
    ("array_bounds",
     {"type": "array", "items": {"type": "integer"}, "minItems": 1, "maxItems": 3},
     [[1], [1, 2], [7, -8, 9]],
     [[], [1, 2, 3, 4], ["a"], [1.5], {"a": 1}]),
    ("array_max_only",
     {"type": "array", "items": {"type": "boolean"}, "maxItems": 2},
     [[], [True], [True, False]],
     [[True, False, True], [1]]),
    ("string_length",
     {"type": "string", "minLength": 2, "maxLength": 4},
     ["ab", "abcd", "é\"\\"],
     ["a", "abcde", "", 5, None]),
    ("type_list",
     {"type": ["string", "null", "boolean"]},
     ["x", None, True, False],
     [3, [], {}]),
    ("number", {"type": "number"}, [1, -2.5, 1e10, 1.5e-7, 0], ["1", True, None, [1]]),
    ("integer", {"type": "integer"}, [0, -7, 123456789], [1.5, "1", False]),
    ("enum_mixed", {"enum": [1, "a", None, True, [1, 2]]}, [1, "a", None, True, [1, 2]], [2, "b", False, [1], [1, 2, 3]]),
    ("const", {"const": {"a": [1, 2], "b": "x"}}, [{"a": [1, 2], "b": "x"}], [{"a": [1, 2]}, {"a": [1, 2], "b": "y"}, 1]),
    ("any_of",
     {"anyOf": [{"type": "integer"}, {"type": "string", "maxLength": 2}, {"type": "array", "items": {"type": "null"}}]},
     [5, "ab", "", [None, None]],
     ["abc", 1.5, [1], None]),
    ("one_of",
     {"oneOf": [{"type": "boolean"}, {"type": "object", "properties": {"x": {"type": "number"}}, "required": ["x"]}]},
     [True, {"x": 2.5}],
     [{}, {"x": "2"}, "true"]),
    ("refs",
     {"type": "object", "properties": {"child": {"$ref": "#/$defs/node"}, "other": {"$ref": "#/definitions/flag"}},
      "$defs": {"node": NODE}, "definitions": {"flag": {"type": "boolean"}}},
     [{}, {"child": {"v": 1}}, {"child": {"v": 1, "next": {"v": 2, "next": {"v": 3}}}, "other": False}],
     [{"child": {"next": {"v": 2}}}, {"child": {"v": 1, "next": {}}}, {"other": 1}, {"child": 1}]),
    ("additional_schema",
     {"type": "object", "properties": {"b": {"type": "integer"}, "bb": {"type": "null"}}, "required": ["b"],
      "additionalProperties": {"type": "boolean"}},
     [{"b": 1}, {"a": True, "b": 1, "c": False}, {"b": 1, "ba": True, "bb": None, "bbb": False, "": True}],
     [{"a": 1, "b": 1},                                # an extra key of the wrong type
      {"a": True},                                     # b is missing
      {"b": True},                                     # b must be an integer, not an extra key
      {"b": 1, "bb": True}]),
    ("additional_true",
     {"type": "object", "additionalProperties": True},
     [{}, {"x": [1, {"y": None}], "z": "s"}],
     [[], 1]),
    ("nested_optional",
     {"type": "array", "maxItems": 2,
      "items": {"type": "object", "required": ["b"],
                "properties": {"a": {"type": "boolean"}, "b": {"type": "null"}, "c": {"type": "string"}}}},
     [[], [{"b": None}], [{"a": True, "b": None, "c": "x"}, {"b": None, "c": ""}], [{"a": False, "b": None}]],
     [[{"a": True}], [{"b": None, "c": 1}], [{"b": None}] * 3, [{"b": None, "d": 1}]]),
]


def _dumps(v):
    return json.dumps(v, sort_keys=True, separators=(",", ":"))


def _accepts(g, text):
    st = g.state()
    return st.accept_text(text) and st.can_end


@pytest.mark.parametrize("name,schema,valid,invalid", CASES, ids=[c[0] for c in CASES])
def test_instances(native, name, schema, valid, invalid):
    from mipipe.grammar import Grammar
    g = Grammar(json_schema=schema)
    for v in valid:
        assert _accepts(g, _dumps(v)), (name, _dumps(v), g.gbnf)
    for v in invalid:
        assert not _accepts(g, _dumps(v)), (name, _dumps(v))


def test_every_supported_keyword_is_covered():
    seen = set()

    def walk(s):
        if isinstance(s, dict):
            seen.update(s)
            for v in s.values():
                walk(v)
        elif isinstance(s, list):
            for v in s:
                walk(v)

    for _, schema, _, _ in CASES:
        walk(schema)
    assert {"type", "properties", "required", "additionalProperties", "items", "minItems", "maxItems", "enum", "const",
            "minLength", "maxLength", "anyOf", "oneOf", "$ref", "$defs", "definitions"} <= seen


def test_whitespace_is_optional_and_bounded(native):
    from mipipe.grammar import Grammar
    g = Grammar(json_schema=CASES[0][1])
    assert _accepts(g, '{ "age" : 3 ,\n "kind" : "a" }')
    assert _accepts(g, json.dumps({"age": 3, "kind": "a"}, sort_keys=True))          # the default separators
    assert not _accepts(g, '{"age":' + " " * 40 + '3,"kind":"a"}')
    st = g.state()
    assert st.accept_text("{")
    n = 0
    while st.accept_text(" "):                     # a model that likes blanks runs out of them
        n += 1
        assert n < 100
    assert 1 <= n < 100


UNSUPPORTED = [("pattern", {"type": "string", "pattern": "^a+$"}), ("format", {"type": "string", "format": "date"}),
               ("allOf", {"allOf": [{"type": "string"}]}), ("not", {"not": {"type": "null"}}),
               ("if", {"if": {"type": "string"}, "then": {"minLength": 1}}),
               ("patternProperties", {"type": "object", "patternProperties": {"^x": {}}}),
               ("minimum", {"type": "integer", "minimum": 0}), ("maximum", {"type": "number", "maximum": 1}),
               ("exclusiveMinimum", {"type": "number", "exclusiveMinimum": 0}), ("multipleOf", {"type": "integer", "multipleOf": 2}),
               ("uniqueItems", {"type": "array", "uniqueItems": True}), ("prefixItems", {"type": "array", "prefixItems": [{}]}),
               ("minProperties", {"type": "object", "minProperties": 1}), ("propertyNames", {"type": "object", "propertyNames": {}}),
               ("contains", {"type": "array", "contains": {"type": "integer"}}),
               ("minimum", {"type": "object", "properties": {"deep": {"type": "array", "items": {"minimum": 3}}}})]


@pytest.mark.parametrize("keyword,schema", UNSUPPORTED, ids=[f"{k}{i}" for i, (k, _) in enumerate(UNSUPPORTED)])
def test_unsupported_keywords_are_named(native, keyword, schema):
    from mipipe.grammar import json_schema_to_gbnf
    with pytest.raises(RuntimeError, match=f'"{keyword}"'):
        json_schema_to_gbnf(schema)


def test_other_refusals(native):
    from mipipe.grammar import json_schema_to_gbnf
    for schema, what in [({"$ref": "http://example.com/x"}, r"\$ref"), ({"$ref": "#/$defs/missing"}, "names nothing"),
                         ({"type": "object", "required": ["a"]}, "not in properties"),
                         ({"type": "array", "items": [{"type": "integer"}]}, "items"),
                         ({"type": "colour"}, "colour"), ({"type": "string", "maxItems": 2}, "array keywords")]:
        with pytest.raises(RuntimeError, match=what):
            json_schema_to_gbnf(schema)


def test_json_object(native):
    from mipipe.grammar import Grammar
    g = Grammar(json_schema={"type": "json_object"})
    for doc in ({}, {"a": 1}, {"a": {"b": [1, 2.5, -3e-4, "x", None, True, {"c": []}]}, "d": "é☃ \"q\" \\ \n"}):
        assert _accepts(g, _dumps(doc)), doc
        assert _accepts(g, json.dumps(doc, indent=1, ensure_ascii=False)), doc
    for text in ("[1,2]", '{"a":1,}', '{"a":1', '{a:1}', '{"a":01}', '{"a":"\t"}', '{"a":1} ', "null", '{"a":1}{"b":2}'):
        assert not _accepts(g, text), text
    st = g.state()
    assert st.accept_text('{"a":[1,{"b":null}]}') and st.only_end
