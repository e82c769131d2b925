"""Host-side checks (no GPU) of the co-hosted launches of an 'mlp8' expert: the W8 guest kinds and their argument struct mirror include/vlaser_hip.h, the library exports
the looped W8 down projection, and that entry refuses bad arguments on the host, before any launch."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, 'include', 'vlaser_hip.h')).read()


def _named_struct_fields(name):
    """field names of `typedef struct NAME { ... } NAME;` in declaration order"""
    body = re.search(r'typedef struct ' + name + r' \{(.*?)\} ' + name + ';', _header(), flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for stmt in body.split(';'):
        for part in stmt.split(','):
            ident = re.findall(r'(\w+)\s*$', part.strip().replace('*', ' '))
            if ident:
                fields.append(ident[0])
    return fields


def test_library_exports_the_looped_w8_entry():
    from vlaser_amd import _lib
    lib = _lib.lib()
    assert 'vlaser_chain_down_looped_w8' in _lib._SIGS and hasattr(lib, 'vlaser_chain_down_looped_w8')
    assert re.search(r'\bint\s+vlaser_chain_down_looped_w8\s*\(', _header())
    assert lib.vlaser_abi_version() == 8          # purely additive


def test_guest_kinds_and_w8_struct_mirror_header():
    from vlaser_amd import _lib
    h = _header()
    kinds = dict(re.findall(r'\b(VL_GUEST_\w+)\s*=\s*(\d+)', h))
    assert kinds['VL_GUEST_CHAIN_GU_W8'] == '6' and kinds['VL_GUEST_CHAIN_DOWN_W8'] == '7'
    for name, val in kinds.items():
        assert getattr(_lib, name[3:]) == int(val), name
    # the existing struct kept its layout; the new one is its fields plus the scales
    down = _named_struct_fields('VlaserChainDownArgs')
    assert down == ['x', 'ldx', 'W', 'res', 'h_out', 'M', 'N', 'K', 'dbg'] == [f[0] for f in _lib.ChainDownArgs._fields_]
    down8 = _named_struct_fields('VlaserChainDownW8Args')
    assert down8 == down + ['w_scale'] == [f[0] for f in _lib.ChainDownW8Args._fields_]
    for a, b in zip(_lib.ChainDownArgs._fields_, _lib.ChainDownW8Args._fields_):
        assert a == b and getattr(_lib.ChainDownArgs, a[0]).offset == getattr(_lib.ChainDownW8Args, a[0]).offset


def test_looped_w8_bad_arguments_return_errors_not_crashes():
    """Argument validation happens on the host before any launch: exercised without a GPU (no call below has a valid argument set, so none reaches a launch)."""
    from vlaser_amd import _lib
    lib = _lib.lib()
    P = 4096
    looped = lambda x=P, ldx=8960, W=P, sc=P, res=P, out=2 * P, M=5, N=768, K=8960: lib.vlaser_chain_down_looped_w8(x, ldx, W, sc, res, out, M, N, K, None)
    assert looped(sc=None) != 0 and b'null w_scale' in lib.vlaser_last_error()
    assert looped(sc=P + 4) != 0 and b'alignment' in lib.vlaser_last_error()
    assert looped(M=4) != 0 and b'looped' in lib.vlaser_last_error()              # one row group: the stand-alone kernel's shape
    assert looped(M=9) != 0 and b'looped' in lib.vlaser_last_error()
    assert looped(N=774) != 0 and b'looped' in lib.vlaser_last_error()            # 258 units of 3 columns: 4 does not divide them
    assert looped(N=772) != 0 and b'looped' in lib.vlaser_last_error()            # 4-column units
    assert looped(W=None) != 0 and b'null' in lib.vlaser_last_error()
    assert looped(W=P + 8) != 0 and b'alignment' in lib.vlaser_last_error()
    assert looped(K=18944) != 0 and b'built for' in lib.vlaser_last_error()
    assert looped(out=P) != 0                                                     # res == h_out
    # the bf16 entry answers as before
    assert lib.vlaser_chain_down_looped(P, 8960, P, P, 2 * P, 4, 768, 8960, None) != 0 and b'looped' in lib.vlaser_last_error()
