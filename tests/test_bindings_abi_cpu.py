"""The three hand-written copies of the C ABI agree, argument by argument (CPU): include/ohxgb.h, the interface blocks
of quickchem_amd/fortran/ohx_bindings.F90 and the argtypes of quickchem_amd/capi.py.  The parsers and the comparison
are tests/bindings_support.py; what cannot be classified fails.

A Fortran dummy stands for a C parameter when
    int, unsigned, int32_t by value        integer(c_int) or integer(c_int32_t), value
    float by value                         real(c_float), value
    bst_ulong, uint64_t, int64_t by value  integer(c_int64_t), value
    a handle or any pointer                type(c_ptr), value; or a dummy WITHOUT value whose type is the pointee's
                                           (float* - a scalar or an array of real(c_float); char* - character(kind=c_char))
    T**, or a handle by reference          type(c_ptr) without value
    void* by reference                     the communicator id only (VOID_BY_REFERENCE)
and carries the header's parameter name (RENAMED lists the four that do not): the name is what tells two neighbours of
one type apart, eta from lambda.  The result is integer(c_int) for int and type(c_ptr) for a pointer.

For ctypes: as many argtypes as parameters; a scalar of the same kind, signedness and width; a pointer-like type for
every pointer, and for POINTER(T) a T of the pointee's kind and width.

test_a_changed_block_is_rejected feeds the comparison changed copies of the bindings text, made in memory: the check
can fail.  No file is written."""
import ctypes as C
import os
import subprocess

import pytest

from quickchem_amd import capi
from tests import bindings_support as B
from tests import helpers

HEADER = os.path.join(helpers.ROOT, "include", "ohxgb.h")
BINDINGS = os.path.join(helpers.ROOT, "quickchem_amd", "fortran", "ohx_bindings.F90")
TRAIN_DRIVER = os.path.join(helpers.ROOT, "quickchem_amd", "lib", "train_driver_hip")

# blocks whose Fortran name is not the C name: both are private to the module and serve ohx_last_error
OTHER_NAME = {"XGBGetLastError_c": "XGBGetLastError", "c_strlen": "strlen"}
NOT_IN_THE_HEADER = ("strlen",)
# dummies that go by another name than the header's parameter: the reference's own names in XGBoosterPredict
# (Shared/xgb_fortran_api.F90), `value` is an attribute in Fortran, and `comm` says what comes out
RENAMED = {("XGBoosterPredict", "length"): "out_len", ("XGBoosterPredict", "prediction"): "out_result",
           ("XGBoosterSetParam", "val"): "value", ("OHXCommInitRank", "comm"): "out"}
# void* taken by reference: the 128 bytes of the communicator id, a character array
VOID_BY_REFERENCE = (("OHXCommGetUniqueId", "id"), ("OHXCommInitRank", "id"))
# header symbols without an interface block: a new symbol in the header has to be put here or be given a block
UNBOUND = [
    "OHXBoosterCheck", "OHXBoosterCopyEngineChoice", "OHXBoosterGetInfo", "OHXBoosterGetNumGroups",
    "OHXBoosterKernelSymbol", "OHXBoosterKernelSymbolRows", "OHXBoosterPredictContribsDevice", "OHXBoosterPredictDevice",
    "OHXBoosterPredictFieldsDevice", "OHXBoosterPredictInteractionsDevice", "OHXBoosterRingReruns", "OHXBoosterRun1",
    "OHXBoosterRun1Device", "OHXDMatrixGetGrid", "OHXDMatrixInferGrid", "OHXDeviceCount", "OHXJulianDay",
    "OHXOHPostProcess", "OHXOHPostProcessDevice", "OHXReleaseScratch", "OHXSolarGeometry", "OHXSolarGeometryDevice",
    "OHXUnregisterHost", "XGBoosterLoadModelFromBuffer", "XGDMatrixCreateFromFile", "XGDMatrixSaveBinary",
]
# what tests/fortran/train_driver.F90 calls, beside the predict path
TRAINING = (["OHXQuantileCuts", "OHXDMatrixQuantileCuts", "OHXDMatrixCreateFromDevice", "OHXBoosterRefitLeaves",
             "OHXBoosterRefitLeavesDevice", "OHXBoosterCountVisits", "OHXBoosterCountVisitsDevice",
             "OHXBoosterGetVisitCounts", "OHXBoosterResetVisitCounts", "OHXBoosterRefreshCover",
             "OHXBoosterPredictContribs", "OHXBoosterPredictInteractions", "OHXDMatrixSetGrid",
             "OHXBoosterGetNumCategoricalSplits"] +
            ["OHXBoosterBoostTrees" + kind + form for kind in ("", "Eval", "Weighted", "Sampled", "Deep", "DeepSampled")
             for form in ("", "Device")])

BINDINGS_TEXT = open(BINDINGS).read()
PROTOS = B.parse_header(open(HEADER).read())
BLOCKS = B.parse_bindings(BINDINGS_TEXT)


def disagreements(blocks, name):
    block = blocks[name]
    out = []
    if OTHER_NAME.get(name, name) != block.bind:
        out.append(f"function {name} binds {block.bind}")
    if block.bind in NOT_IN_THE_HEADER:
        return out
    if block.bind not in PROTOS:
        return out + [f"{block.bind} is not in the header"]
    return out + B.compare_block(block, PROTOS[block.bind], RENAMED, VOID_BY_REFERENCE)


# ---- the parsers ----

def test_the_header_parses_into_every_prototype():
    assert len(PROTOS) == 78
    assert sorted(PROTOS) == sorted(capi.ABI_SYMBOLS)
    p = PROTOS["OHXBoosterPredictContribsFields"]
    kinds = {q.name: q.type for q in p.params}
    assert kinds["fields"] == B.CType("float", 4, 2)               # const float* const fields[]
    assert kinds["is2d"] == B.CType("int", 4, 1) and kinds["out"] == B.CType("float", 4, 2)
    assert kinds["handle"] == B.CType("void", 0, 1) and kinds["ntree_limit"] == B.CType("uint", 4, 0)
    assert PROTOS["XGBGetLastError"].ret == B.CType("char", 1, 1) and PROTOS["XGBGetLastError"].params == []
    assert PROTOS["OHXCommInitRank"].params[3].type == B.CType("void", 0, 2)          # OHXCommHandle* out
    assert PROTOS["OHXBoosterGetInfo"].params[1].type == B.CType("uint", 8, 1)        # bst_ulong info[8]
    assert [q.name for q in PROTOS["OHXBoosterBoostTrees"].params[8:12]] == ["eta", "lambda", "gamma", "min_child_rows"]


@pytest.mark.parametrize("text", ["int f(long x);", "int f(struct S* s);", "int f(float);", "int g(int a) { return a; }",
                                  "void f(int a);", "int f(int a); int f(int a);", "int f(char c);"])
def test_what_the_header_parser_cannot_classify_is_an_error(text):
    with pytest.raises(B.Unparsed):
        B.parse_header(text)


def test_the_bindings_parse_into_every_block():
    assert len(BLOCKS) == 53
    b = BLOCKS["OHXBoosterBoostTreesSampledDevice"]
    assert len(b.dummies) == 27 and b.bind == "OHXBoosterBoostTreesSampledDevice"
    by_name = {d.name: d for d in b.dummies}
    assert by_name["cut_ptr"] == B.FDummy("cut_ptr", "integer", "c_int64_t", False, True)
    assert by_name["patience"] == B.FDummy("patience", "integer", "c_int", True, False)
    assert by_name["rounds_run"] == B.FDummy("rounds_run", "integer", "c_int", False, False)
    assert by_name["stream"] == B.FDummy("stream", "type", "c_ptr", True, False)
    assert [d.name for d in b.dummies[:3]] == ["handle", "dmat", "d_labels"] and b.dummies[-1].name == "stream"
    assert b.result == B.FDummy("rc", "integer", "c_int", False, False)
    assert BLOCKS["XGBoosterSetParam"].dummies[1] == B.FDummy("name", "character", "c_char", False, True)


@pytest.mark.parametrize("text", [
    'function f(a) bind(C, name="f") result(rc)\n integer(c_int) :: rc\n end function',                     # a undeclared
    'function f(a) bind(C, name="f") result(rc)\n integer(c_int) :: a, b, rc\n end function',               # b no dummy
    'function f(a) bind(C, name="f") result(rc)\n integer(c_int), optional :: a\n integer(c_int) :: rc\n end function',
    'function f(a) bind(C, name="f") result(rc)\n integer(c_int) :: a, rc\n',                               # no end
    'integer(c_int) function f(a) bind(C, name="f")\n integer(c_int) :: a\n end function',                  # another form
])
def test_what_the_bindings_parser_cannot_classify_is_an_error(text):
    with pytest.raises(B.Unparsed):
        B.parse_bindings(text)


def test_comments_and_continuations():
    text = ('function f(a, & ! the first\n      & b) bind(C, name="f") &\n   result(rc)\n'
            '   real(c_float), value :: a ! b is next\n   character(kind=c_char), intent(in) :: b(*)\n'
            '   integer(c_int) :: rc\nend function f\n')
    f = B.parse_bindings(text)["f"]
    assert [d.name for d in f.dummies] == ["a", "b"] and f.dummies[1].array and f.dummies[0].value


# ---- ohx_bindings against the header ----

@pytest.mark.parametrize("name", sorted(BLOCKS))
def test_block_agrees_with_the_header(name):
    assert disagreements(BLOCKS, name) == []


def test_header_symbols_without_a_block():
    assert len(UNBOUND) == 26
    bound = {b.bind for b in BLOCKS.values()}
    assert sorted(set(PROTOS) - bound) == sorted(UNBOUND)
    assert "OHXDMatrixCreateFromDevice" in bound


def test_every_block_can_be_used():
    """The module is private: a block a caller is to reach has to be named in a public statement."""
    public = set()
    for stmt in B.fortran_lines(BINDINGS_TEXT):
        if stmt.lower().startswith("public"):
            public |= {n.strip() for n in stmt.split("::")[1].split(",")}
    assert sorted(set(BLOCKS) - public) == sorted(OTHER_NAME)
    assert set(TRAINING) <= public


def in_block(name, pattern, repl):
    return lambda text: B.edit_block(text, name, pattern, repl)


SAMPLED, EVAL, PLAIN = "OHXBoosterBoostTreesSampledDevice", "OHXBoosterBoostTreesEval", "OHXBoosterBoostTreesDevice"
# (what is changed, the block, the change, a word the complaint must hold)
CHANGES = [
    ("a value removed from patience", SAMPLED,
     in_block(SAMPLED, r"(:: rounds, max_depth), patience", r"\1\n integer(c_int) :: patience"), "patience"),
    ("a value added to rounds_run", EVAL,
     in_block(EVAL, r"integer\(c_int\), intent\(out\)( +):: rounds_run, best_round",
              r"integer(c_int), value :: rounds_run\n integer(c_int), intent(out) :: best_round"), "rounds_run"),
    ("eta and lambda swapped in the function statement", PLAIN,
     in_block(PLAIN, r"max_depth, eta, &\s*lambda, gamma", "max_depth, lambda, eta, gamma"), "eta"),
    ("nlabel declared integer(c_int)", EVAL,
     in_block(EVAL, r"integer\(c_int64_t\), value( +):: nlabel, eval_nlabel",
              r"integer(c_int), value :: nlabel\n integer(c_int64_t), value :: eval_nlabel"), "nlabel"),
    ("min_child_weight declared real(c_double)", SAMPLED,
     in_block(SAMPLED, r"gamma, min_child_weight, subsample, colsample_bytree\n",
              "gamma, subsample, colsample_bytree\n real(c_double), value :: min_child_weight\n"), "min_child_weight"),
    ("one dummy deleted", PLAIN,
     in_block(PLAIN, r"lambda, gamma, min_child_rows, nodes_added, stream\)(.*?):: eta, lambda, gamma\n",
              r"lambda, min_child_rows, nodes_added, stream)\1:: eta, lambda\n"), "parameters"),
    ("stream moved to the front", SAMPLED,
     in_block(SAMPLED, r"\(handle, dmat, (.*?), &(\s*)stream\) bind", r"(stream, handle, dmat, \1) &\2bind"), "nlabel"),
    ("cut_ptr declared real(c_float)", EVAL,
     in_block(EVAL, r"integer\(c_int64_t\), intent\(in\)( +):: cut_ptr\(\*\)", r"real(c_float), intent(in) :: cut_ptr(*)"),
     "cut_ptr"),
    ("seed declared integer(c_int)", SAMPLED,
     in_block(SAMPLED, r"integer\(c_int64_t\), value( +):: seed", "integer(c_int), value :: seed"), "seed"),
    ("min_child_rows declared integer(c_int)", PLAIN,
     in_block(PLAIN, r"integer\(c_int64_t\), value( +):: min_child_rows", "integer(c_int), value :: min_child_rows"),
     "min_child_rows"),
    ("train_rmse by reference", EVAL,
     in_block(EVAL, r"type\(c_ptr\), value( +):: train_rmse, eval_rmse",
              "type(c_ptr) :: train_rmse\n type(c_ptr), value :: eval_rmse"), "train_rmse"),
    ("patience and rounds exchanged in the function statement", EVAL,
     in_block(EVAL, r"cut_values, rounds, max_depth, (.*?), patience, train_rmse",
              r"cut_values, patience, max_depth, \1, rounds, train_rmse"), "rounds"),
    ("the result declared integer(c_int64_t)", PLAIN,
     in_block(PLAIN, r"integer\(c_int\)( +):: rc", "integer(c_int64_t) :: rc"), "result"),
    ("bound to another symbol", PLAIN,
     in_block(PLAIN, r'name="OHXBoosterBoostTreesDevice"', 'name="OHXBoosterBoostTrees"'), "binds"),
]


@pytest.mark.parametrize("what,name,change,word", CHANGES, ids=[c[0] for c in CHANGES])
def test_a_changed_block_is_rejected(what, name, change, word):
    assert disagreements(BLOCKS, name) == []
    changed = change(BINDINGS_TEXT)
    assert changed != BINDINGS_TEXT
    blocks = B.parse_bindings(changed)
    found = disagreements(blocks, name)
    assert found and any(word in line for line in found), (what, found)
    # and nothing else: every other block still agrees
    assert [n for n in blocks if n != name and disagreements(blocks, n)] == []
    assert open(BINDINGS).read() == BINDINGS_TEXT


# ---- capi.py against the header ----

@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


@pytest.mark.parametrize("name", capi.ABI_SYMBOLS)
def test_argtypes_agree_with_the_header(lib, name):
    fn = getattr(lib, name)
    assert B.compare_ctypes(name, fn.argtypes, fn.restype, PROTOS[name]) == []


def test_changed_argtypes_are_rejected(lib):
    name = "OHXBoosterBoostTreesSampled"
    good = list(getattr(lib, name).argtypes)
    proto = PROTOS[name]
    assert B.compare_ctypes(name, good, C.c_int, proto) == []
    at = {p.name: n for n, p in enumerate(proto.params)}

    def with_(param, t):
        out = list(good)
        out[at[param]] = t
        return out
    for param, t in (("nlabel", C.c_int), ("nlabel", C.c_int64), ("seed", C.c_uint32), ("eta", C.c_double),
                     ("patience", C.c_float), ("patience", C.c_uint), ("rounds_run", C.c_int), ("rounds_run", C.POINTER(C.c_int64)),
                     ("rounds_run", C.POINTER(C.c_float)), ("nodes_added", C.POINTER(C.c_int)), ("labels", C.c_uint64),
                     ("labels", C.c_char_p), ("handle", C.POINTER(C.POINTER(C.c_float)))):
        found = B.compare_ctypes(name, with_(param, t), C.c_int, proto)
        assert len(found) == 1 and f"({param})" in found[0], (param, t, found)
    assert B.compare_ctypes(name, good[:-1], C.c_int, proto) and B.compare_ctypes(name, good + [C.c_void_p], C.c_int, proto)
    assert B.compare_ctypes(name, None, C.c_int, proto)
    assert B.compare_ctypes(name, good, C.c_int64, proto) and B.compare_ctypes(name, good, C.c_char_p, proto)
    assert B.compare_ctypes(name, good, None, proto)
    # T** against POINTER(POINTER(T)), char** against POINTER(c_char_p)
    predict = PROTOS["XGBoosterPredict"]
    good = list(lib.XGBoosterPredict.argtypes)
    assert B.compare_ctypes("XGBoosterPredict", good[:-1] + [C.POINTER(C.c_float)], C.c_int, predict)
    assert B.compare_ctypes("XGBoosterPredict", good[:-1] + [C.POINTER(C.POINTER(C.c_double))], C.c_int, predict)
    assert B.compare_ctypes("XGBGetLastError", [], C.c_int, PROTOS["XGBGetLastError"])


# ---- the driver that calls the training family from Fortran ----

def test_train_driver_is_built_against_the_product_only():
    assert os.path.exists(TRAIN_DRIVER), TRAIN_DRIVER
    out = subprocess.run(["ldd", TRAIN_DRIVER], stdout=subprocess.PIPE, text=True).stdout
    assert "libohxgb.so" in out and "libamdhip64" in out and "oracle" not in out
    nm = subprocess.run(["nm", "-D", "--undefined-only", TRAIN_DRIVER], stdout=subprocess.PIPE, text=True).stdout
    undefined = {ln.split()[-1].split("@")[0] for ln in nm.splitlines() if ln.strip()}
    assert len(TRAINING) == 26 and set(TRAINING) <= undefined
    assert {s for s in undefined if s.startswith("hip")} == {"hipMalloc", "hipMemcpy", "hipFree", "hipDeviceSynchronize"}
    # the oracle-linked drivers link ohx_bindings.o too: the interface blocks alone must not pull a symbol in
    obj = os.path.join(helpers.ROOT, "quickchem_amd", "lib", "obj", "ohx_bindings.o")
    nm = subprocess.run(["nm", "--undefined-only", obj], stdout=subprocess.PIPE, text=True).stdout
    assert not [s for s in TRAINING if s in nm]
