"""Structure figures of the attention host code: code lines (non-blank, non-comment, non-docstring) of the files given
(bevrender_amd/ops.py first, the SCA module second), of _AttnCore.forward / .backward and attention_core, what _AttnCore
still derives itself, and how often each attention entry point's name occurs in ops.py outside comments and docstrings.

    python tools/code_lines.py bevrender_amd/ops.py bevrender_amd/model/SCA_deform_attn.py"""
import ast, io, re, sys, tokenize
def code_lines(src):
    """line numbers holding code: non-blank, non-comment, non-docstring"""
    doc = set()
    for n in ast.walk(ast.parse(src)):
        if isinstance(n, (ast.Module, ast.ClassDef, ast.FunctionDef)) and n.body and isinstance(n.body[0], ast.Expr) \
                and isinstance(getattr(n.body[0], "value", None), ast.Constant) and isinstance(n.body[0].value.value, str):
            doc.update(range(n.body[0].lineno, n.body[0].end_lineno + 1))
    lines = set()
    for t in tokenize.generate_tokens(io.StringIO(src).readline):
        if t.type not in (tokenize.COMMENT, tokenize.NL, tokenize.NEWLINE, tokenize.INDENT, tokenize.DEDENT, tokenize.ENDMARKER):
            lines.update(range(t.start[0], t.end[0] + 1))
    return lines - doc
def report(path_ops, path_sca):
    tot = 0
    for p in (path_ops, path_sca):
        src = open(p).read(); n = len(code_lines(src)); tot += n; print(p, n)
    print("total code lines", tot)
    src = open(path_ops).read(); cl = code_lines(src); L = src.split("\n")
    tree = ast.parse(src)
    for n in ast.walk(tree):
        if isinstance(n, ast.ClassDef) and n.name == "_AttnCore":
            for f in n.body:
                if isinstance(f, ast.FunctionDef): print("_AttnCore." + f.name, len([i for i in range(f.lineno, f.end_lineno + 1) if i in cl]), "code lines;", f.end_lineno - f.lineno + 1, "lines")
            body = "\n".join(L[i - 1] for i in range(n.lineno, n.end_lineno + 1) if i in cl)
            print("_AttnCore mentions:", {k: body.count(k) for k in ("gather_supported", "slab_supported", "os.environ")})
        if isinstance(n, ast.FunctionDef) and n.name == "attention_core":
            print("attention_core", len([i for i in range(n.lineno, n.end_lineno + 1) if i in cl]), "code lines;", n.end_lineno - n.lineno + 1, "lines")
    code = "\n".join(re.sub(r"#.*", "", L[i - 1]) for i in sorted(cl))
    names = sorted(set(re.findall(r"bevr_attn_\w+|bevr_kv_project|bevr_pack_kv|bevr_unpack_dkv", code)))
    print("entry point occurrences in code:", {k: len(re.findall(r"\b%s\b" % k, code)) for k in names})
    sca = open(path_sca).read()
    print("_pinned_keys_tap( calls in SCA:", len(re.findall(r"self\._pinned_keys_tap\(", sca)))
report(sys.argv[1], sys.argv[2])
