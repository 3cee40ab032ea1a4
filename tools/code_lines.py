#!/usr/bin/env python3
"""Count the code lines of a region of a Python file: lines that hold a token other than a comment, outside docstrings.

    tools/code_lines.py FILE [FROM_TEXT TO_TEXT]

The region runs from the line that holds FROM_TEXT to the line before the one that holds TO_TEXT; the default is the
decode region of flash_attention.py, from the "Ragged few-query forward" banner through ``_append_call``."""
import ast
import io
import sys
import tokenize as T


def code_lines(src, start="# Ragged few-query forward", stop="# Op-name mirror"):
    lo, hi = src[:src.index(start)].count("\n"), src[:src.index(stop)].count("\n")
    doc = {n for d in ast.walk(ast.parse(src)) if isinstance(d, (ast.FunctionDef, ast.ClassDef)) and ast.get_docstring(d)
           for n in range(d.body[0].lineno, d.body[0].end_lineno + 1)}
    skip = (T.COMMENT, T.NL, T.NEWLINE, T.INDENT, T.DEDENT, T.ENDMARKER)
    code = {n for t in T.generate_tokens(io.StringIO(src).readline) if t.type not in skip
            for n in range(t.start[0], t.end[0] + 1)}
    return len([n for n in code - doc if lo < n <= hi])


if __name__ == "__main__":
    if len(sys.argv) not in (2, 4):
        sys.exit(__doc__)
    print(code_lines(open(sys.argv[1]).read(), *sys.argv[2:]))
