"""Source scan that holds the stream arguments of the library's host code in place without a GPU (DESIGN.md "Stream
contract"; tests/test_gpu_streams.py is the behavioural side).  Over marl_llm_amd/csrc/*.hip but legacy_shim.hip, whose five
symbols are synchronous null-stream calls by contract:

  1. every hipLaunchKernelGGL, hipMemcpyAsync and hipMemsetAsync passes a stream that is an expression, not 0 / nullptr / NULL,
     and no kernel is launched with the <<< >>> syntax (whose stream is optional);
  2. the plain hipMemcpy / hipMemcpy2D / hipMemset calls -- null-stream work -- are exactly PLAIN_CALLS below;
  3. the side kernels' launchers (launch_*) are handed a stream that is not the null stream;
  4. where such a plain call sits in a function that can run with work in flight, a hipStreamSynchronize(h->stream) precedes it.

Adding a null-stream call means editing PLAIN_CALLS in the same change, with the reason it is safe there.
"""
import glob
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "marl_llm_amd", "csrc")
NULL_STREAMS = {"0", "nullptr", "NULL", "hipStreamDefault", "(hipStream_t)0", "hipStream_t()", "hipStream_t{}"}
STREAM_ARG = {"hipLaunchKernelGGL": 4, "hipMemcpyAsync": 4, "hipMemsetAsync": 3, "hipMemcpy2DAsync": 7}       # 0-based
PLAIN = ("hipMemcpy", "hipMemcpy2D", "hipMemset")

# (file, enclosing function, call) -> count, and why the null stream is safe there
PLAIN_CALLS = {
    ("env_api.hip", "swarm_create", "hipMemset"): 1,        # fills of fresh buffers; the function ends with hipStreamSynchronize(nullptr)
    ("env_api.hip", "io_alloc", "hipMemset"): 1,            # the same, of the fresh export block
    ("env_api.hip", "swarm_set_cells", "hipMemcpy"): 2,     # behind the function's own hipStreamSynchronize(h->stream)
    ("env_api.hip", "swarm_set_shapes", "hipMemcpy"): 5,    # into buffers allocated aside that no enqueued work knows yet
    ("env_api.hip", "swarm_path_envs", "hipMemcpy2D"): 1,   # behind the function's own hipStreamSynchronize(h->stream)
    ("swarm_env.hip", "swarm_debug_stamps", "hipMemset"): 1,         # SWARM_STAMPS builds only (diagnostic)
    ("swarm_env.hip", "swarm_debug_stamps", "hipMemcpy"): 1,
}
SYNC_FIRST = [("env_api.hip", "swarm_set_cells"), ("env_api.hip", "swarm_path_envs")]


def strip_code(text):
    """Comments, string / character literals and preprocessor lines blanked out (offsets and line breaks kept)."""
    out, i, n = [], 0, len(text)
    while i < n:
        c = text[i]
        if text.startswith("//", i):
            j = text.find("\n", i); j = n if j < 0 else j
            out.append(" " * (j - i)); i = j
        elif text.startswith("/*", i):
            j = text.find("*/", i + 2); j = n if j < 0 else j + 2
            out.append(re.sub(r"[^\n]", " ", text[i:j])); i = j
        elif c in "\"'":
            j = i + 1
            while j < n and text[j] != c:
                j += 2 if text[j] == "\\" else 1
            out.append(c + " " * (j - i - 1) + c); i = j + 1
        else:
            out.append(c); i += 1
    code = "".join(out)
    return "\n".join(" " * len(l) if l.lstrip().startswith("#") else l for l in code.split("\n"))


def call_args(code, open_paren):
    """The top-level arguments of the call whose '(' is at code[open_paren], and the offset just past its ')'."""
    depth, args, start = 0, [], open_paren + 1
    for i in range(open_paren, len(code)):
        c = code[i]
        if c in "([{":
            depth += 1
        elif c in ")]}":
            depth -= 1
            if depth == 0:
                args.append(code[start:i].strip())
                return args, i + 1
        elif c == "," and depth == 1:
            args.append(code[start:i].strip()); start = i + 1
    raise AssertionError("unbalanced call")


def functions(code):
    """[(name, body start, body end)] of the function definitions of a stripped source: blocks at namespace / extern level
    (or directly inside a struct) whose header has a parameter list.  Lambdas and blocks inside a function belong to it."""
    res, stack, last = [], [], 0               # stack of (kind, name, start); last: offset after the previous ; { or }
    for m in re.finditer(r"[;{}]", code):
        i, c = m.start(), m.group()
        if c == "{":
            head = code[last:i]
            inside_fn = any(k == "fn" for k, _, _ in stack)
            if inside_fn:
                kind, name = "block", None
            elif re.search(r"\b(namespace|extern)\b", head) and "(" not in head:
                kind, name = "open", None
            elif re.search(r"\b(struct|class|union|enum)\b", head) and "(" not in head.split(":")[0]:
                kind, name = "open", None
            elif "(" in head:
                h = re.sub(r"\b__launch_bounds__\s*\([^)]*\)|\b__attribute__\s*\(\([^)]*\)\)", " ", head)
                nm = re.search(r"([A-Za-z_]\w*)\s*\(", h)
                kind, name = "fn", nm.group(1) if nm else "?"
            else:
                kind, name = "block", None      # an initialiser list and the like
            stack.append((kind, name, i + 1))
        elif c == "}" and stack:
            kind, name, start = stack.pop()
            if kind == "fn":
                res.append((name, start, i))
        last = i + 1
    return res


def sources():
    files = sorted(f for f in glob.glob(os.path.join(CSRC, "*.hip")) if os.path.basename(f) != "legacy_shim.hip")
    assert len(files) >= 6
    return [(os.path.basename(f), strip_code(open(f).read())) for f in files]


def enclosing(fns, pos):
    for name, a, b in fns:
        if a <= pos < b:
            return name
    return None


def test_scanner_on_a_known_text():
    code = strip_code('''
namespace { struct S { int f(int t) const { hipMemset(p, 0, n); return 0; } }; }
// hipMemcpy(a, b, n, k);
extern "C" {
int g(void *h)
{
    auto l = [&](int q) { hipMemcpy(a, b, n, k); };
    hipLaunchKernelGGL((k<1, 2>), dim3(g), dim3(64), 0, nullptr, x, f(y, z));
    return 0;
}
#ifdef X
int d() { hipMemcpyAsync(a, b, n, kind, h->stream); }
#endif
}''')
    fns = functions(code)
    assert sorted(n for n, _, _ in fns) == ["d", "f", "g"]
    found = [(enclosing(fns, m.start()), m.group(1)) for m in re.finditer(r"\b(hipMemcpy|hipMemset)\s*\(", code)]
    assert found == [("f", "hipMemset"), ("g", "hipMemcpy")]
    m = re.search(r"hipLaunchKernelGGL\s*\(", code)
    args, _ = call_args(code, m.end() - 1)
    assert args[0] == "(k<1, 2>)" and args[4] == "nullptr" and len(args) == 7


def test_every_launch_and_async_copy_names_a_stream():
    n_calls = 0
    for fname, code in sources():
        assert "<<<" not in code, f"{fname}: a <<< >>> launch (its stream argument is optional): use hipLaunchKernelGGL"
        for m in re.finditer(r"\b(%s)\s*\(" % "|".join(STREAM_ARG), code):
            args, _ = call_args(code, m.end() - 1)
            k = STREAM_ARG[m.group(1)]
            line = code.count("\n", 0, m.start()) + 1
            assert len(args) > k, f"{fname}:{line}: {m.group(1)} with {len(args)} arguments: no stream"
            assert args[k].replace(" ", "") not in NULL_STREAMS, f"{fname}:{line}: {m.group(1)} on the null stream ({args[k]!r})"
            n_calls += 1
    assert n_calls >= 30          # the scan saw the library (it holds about forty such calls)


def test_side_kernel_launchers_are_handed_a_stream():
    """The launchers of env_kernels.hip (launch_reset, launch_interleave, launch_export, ...) take the stream first."""
    n_calls = 0
    for fname, code in sources():
        for m in re.finditer(r"\blaunch_[a-z_]+\s*\(", code):
            args, _ = call_args(code, m.end() - 1)
            line = code.count("\n", 0, m.start()) + 1
            assert args[0].replace(" ", "") not in NULL_STREAMS, f"{fname}:{line}: {m.group(0)} on the null stream"
            n_calls += args[0].endswith("stream")
    assert n_calls >= 6


def test_plain_copies_and_fills_are_the_allow_list():
    found = {}
    for fname, code in sources():
        fns = functions(code)
        for m in re.finditer(r"\b(%s)\s*\(" % "|".join(PLAIN), code):
            fn = enclosing(fns, m.start())
            line = code.count("\n", 0, m.start()) + 1
            assert fn is not None, f"{fname}:{line}: {m.group(1)} outside any function"
            key = (fname, fn, m.group(1))
            found[key] = found.get(key, 0) + 1
    assert found == PLAIN_CALLS, ("null-stream calls changed: added/changed %r, gone %r"
                                  % ({k: v for k, v in found.items() if PLAIN_CALLS.get(k) != v},
                                     {k: v for k, v in PLAIN_CALLS.items() if k not in found}))


@pytest.mark.parametrize("fname,fn", SYNC_FIRST, ids=[f for _, f in SYNC_FIRST])
def test_plain_calls_behind_in_flight_work_follow_a_stream_wait(fname, fn):
    code = dict(sources())[fname]
    body = [code[a:b] for name, a, b in functions(code) if name == fn]
    assert len(body) == 1
    first_plain = re.search(r"\b(%s)\s*\(" % "|".join(PLAIN), body[0])
    assert first_plain is not None
    waits = [m.start() for m in re.finditer(r"\bhipStreamSynchronize\s*\(\s*h->stream\s*\)", body[0])]
    assert waits and min(waits) < first_plain.start(), f"{fn}: no hipStreamSynchronize(h->stream) before its first null-stream call"


def test_create_and_io_alloc_wait_for_their_null_stream_fills():
    code = dict(sources())["env_api.hip"]
    for fn in ("swarm_create", "io_alloc"):
        body = [code[a:b] for name, a, b in functions(code) if name == fn]
        assert len(body) == 1
        fill = [m.start() for m in re.finditer(r"\bhipMemset\s*\(", body[0])]
        wait = [m.start() for m in re.finditer(r"\bhipStreamSynchronize\s*\(\s*nullptr\s*\)", body[0])]
        assert fill and wait and max(wait) > max(fill), fn
