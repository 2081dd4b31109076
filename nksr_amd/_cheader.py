"""Reader for include/nksr_hip.h: the constants, struct layouts and prototypes the ctypes bindings (_lib.py) are built from.

The header is plain C (stddef.h / stdint.h types, no function pointers, unions or bit-fields), so three regular expressions
cover it.  Whatever they do not cover raises HeaderError with the declaration quoted: nothing is guessed, nothing is skipped.

A type is spelled 'int32_t', 'float*', 'nksr_hier_t*': the base name, '*' for a pointer; const and the `struct tag` spelling
of a typedef are dropped."""
import collections
import re

VALUE_TYPES = ('int', 'int32_t', 'int64_t', 'uint64_t', 'size_t', 'float', 'double')           # passed and stored by value
POINTEE_TYPES = VALUE_TYPES + ('void', 'char', 'int8_t', 'uint8_t', 'uint32_t')                # only ever behind a pointer

Header = collections.namedtuple('Header', 'consts structs protos')
# consts {macro: int | float | nested tuples of floats}; structs {typedef: [(field, type, array length or None)]} in declaration
# order; protos {function: (return type, [argument types])}

_DECL = re.compile(r'(?:const\s+)?(struct\s+)?(\w+)\s*(\*?)\s*(?:\b(\w+)\s*(?:\[\s*(\w+)\s*\])?)?')
_MORE = re.compile(r'(\w+)\s*(?:\[\s*(\w+)\s*\])?')            # second and later declarators of `int32_t depth, M;`
_STRUCT = re.compile(r'typedef\s+struct\s*(\w*)\s*\{([^{}]*)\}\s*(\w+)\s*;')
_PROTO = re.compile(r'(.*?)\b(\w+)\s*\(([^()]*)\)')


class HeaderError(ValueError):
    def __init__(self, why, decl):
        ValueError.__init__(self, '%s: `%s`' % (why, ' '.join(decl.split())))


def _const(body, decl):
    """6, (-1), (1ll << 30), {0.01, 0.1}, {{0.5f, 1.0f}, {1.0f, -0.375f}}"""
    py = re.sub(r'(?<=\d)(f|ll)\b', '', body).replace('{', '(').replace('}', ',)')
    if not re.fullmatch(r'[-+\d.e\s,()<]+', py):        # digits and punctuation only: no name can reach eval
        raise HeaderError('not a numeric constant', decl)
    try:
        return eval(py, {'__builtins__': {}})
    except Exception:
        raise HeaderError('not a numeric constant', decl)


def parse(text):
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S).replace('\\\n', ' ')
    consts, structs, protos, tags, code, cxx = {}, {}, {}, {}, [], False
    for line in text.split('\n'):
        if not line.lstrip().startswith('#'):
            if not cxx:
                code.append(line)
        elif re.match(r'\s*#\s*ifdef\s+__cplusplus\s*$', line):       # the extern "C" brackets: not C
            cxx = True
        elif re.match(r'\s*#\s*endif\s*$', line):
            cxx = False
        elif re.match(r'\s*#\s*define\s+\w+\s+\S', line):
            name, body = re.match(r'\s*#\s*define\s+(\w+)\s+(.*)', line).groups()
            consts[name] = _const(body, line)
        elif not re.match(r'\s*#\s*(include\s*<\w+\.h>|ifndef\s+\w+|define\s+\w+)\s*$', line):
            raise HeaderError('unknown preprocessor line', line)

    def typ(decl, m, by_value):
        base = tags.get(m.group(2), m.group(2)) if m.group(1) else m.group(2)
        if m.group(3):
            ok = base in POINTEE_TYPES or base in structs or base in tags.values()
        else:
            ok = base in by_value
        if not ok:
            raise HeaderError('unknown type %s%s' % (base, m.group(3)), decl)
        return base + m.group(3)

    def bound(n, decl):
        n = consts.get(n, n) if n is not None else None
        if n is not None and not str(n).isdigit():
            raise HeaderError('unknown array bound', decl)
        return n if n is None else int(n)

    code = ' '.join(code)
    tags.update((m.group(1), m.group(3)) for m in _STRUCT.finditer(code) if m.group(1))
    for tag, body, name in _STRUCT.findall(code):
        fields = structs[name] = []
        for decl in filter(str.strip, body.split(';')):
            first, *more = [d.strip() for d in decl.split(',')]
            m = _DECL.fullmatch(first)
            if not m or not m.group(4) or (more and m.group(3)) or not all(_MORE.fullmatch(d) for d in more):
                raise HeaderError('cannot split the field declaration', decl)
            t = typ(decl, m, VALUE_TYPES + tuple(s for s in structs if s != name))
            for fname, n in [m.group(4, 5)] + [_MORE.fullmatch(d).groups() for d in more]:
                fields.append((fname, t, bound(n, decl)))
    for decl in filter(str.strip, _STRUCT.sub(' ', code).split(';')):
        if re.fullmatch(r'\s*struct\s+\w+\s*', decl):           # forward declaration of a tag
            if decl.split()[1] not in tags:
                raise HeaderError('struct tag without a typedef', decl)
            continue
        m = _PROTO.fullmatch(decl.strip())
        ret = m and _DECL.fullmatch(m.group(1).strip())
        if not ret or ret.group(4):
            raise HeaderError('cannot split the declaration', decl)
        args = [] if m.group(3).strip() == 'void' else [_DECL.fullmatch(a.strip()) for a in m.group(3).split(',')]
        if not all(args) or any(a.group(5) for a in args):
            raise HeaderError('cannot split the argument list', decl)
        protos[m.group(2)] = (typ(decl, ret, VALUE_TYPES), [typ(decl, a, VALUE_TYPES) for a in args])
    return Header(consts, structs, protos)
