"""What the table tests of the eight bindings share: the element type that snappy.jl_amd/_binding.py
gives every pointer parameter of a *_device function, and every array of a structure of parallel
arrays, against the declaration in include/*.h.  The letters' meaning is written out here, not
taken from the code under test."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LETTERS = {"b": "uint8_t", "w": "uint32_t", "d": "uint64_t", "t": "int32_t"}
STRUCTS = {"smf_chunks": "C", "smb_chunks": "B", "smo_chunks": "O", "smq_pages": "G", "sma_blocks": "A"}


def struct_fields(name):
    """[(element type, field)] of `typedef struct name { ... } name;` in the one header of include/ that has it."""
    include = os.path.join(ROOT, "include")
    found = []
    for header in sorted(os.listdir(include)):
        with open(os.path.join(include, header)) as f:
            found += re.findall(r"typedef struct %s \{(.*?)\} %s;" % (name, name), f.read(), re.S)
    (body,) = found
    return re.findall(r"\b(u?int\d+_t)\s*\*\s*(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))


def assert_struct_elements(binding, name):
    """The structure's fields and their element letters are the header's, in its order."""
    struct = binding.ARRAYS[STRUCTS[name]]
    fields = struct_fields(name)
    assert fields and [n for n, _ in struct._fields_] == [n for _, n in fields], name
    assert [LETTERS[e] for e in struct.elements] == [t for t, _ in fields], name


def assert_device_elements(binding, declared, table):
    """Every pointer parameter of every *_device function of `declared` ({name: (return type,
    [parameter types])}, from a header) has in `table` the letter of its element type; a
    structure's letter stands for the header's structure, whose arrays are compared too; ctx and
    stream alone are plain pointers; and a count mark names a uint32_t parameter.  Returns the
    number of pointer parameters compared."""
    compared = 0
    for name, (_, params) in declared.items():
        if not name.endswith("_device"):
            continue
        letters = binding.arguments(table[name])[1]
        assert len(letters) == len(params), name
        for k, (p, (letter, mark)) in enumerate(zip(params, letters)):
            at = "%s: argument %d (%s) is %r" % (name, k, p.strip(), letter)
            if "*" not in p:
                assert letter not in LETTERS and letter not in STRUCTS.values() and letter != "r" and mark is None, at
                continue
            base = p.replace("const", " ").replace("*", " ").split()[0]
            base = "uint8_t" if base == "char" else base
            if base in LETTERS.values():
                assert LETTERS.get(letter) == base, at
            elif base == "void" or base.endswith("_ctx"):
                assert letter == "p" and k in (0, len(params) - 1), at
            elif base == "smf_summary":
                assert letter == "r", at
            else:
                assert STRUCTS[base] == letter, at
                assert_struct_elements(binding, base)
            if mark is not None and mark[0] is not None:
                count = params[mark[0]]
                assert "*" not in count and count.split() == ["uint32_t"], "%s: its count, argument %d" % (at, mark[0])
            compared += 1
    return compared
