"""The last-workgroup tickets in the compiled code (no GPU): every kernel that closes a reduction in its last workgroup takes
its ticket through csrc/dcr_internal.h::last_arriver, so every wave's payload stores have completed (s_waitcnt vmcnt(0))
before the ticket's atomic add.  Device assembly of the three sources with csrc/build.sh's flags."""
import glob
import os
import re
import shutil
import subprocess

import pytest

from conftest import PKG

CSRC = os.path.join(PKG, 'csrc')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')   # (as build.sh)
MARKER = 'dcr ticket drain'
# source -> {kernel: instantiations}
KERNELS = {
    'dcr_gcn': {'k_picked_mean_fwd': 1, 'k_head_fwd': 3, 'k_head_bwd': 3, 'k_adam_multi': 1},
    'dcr_gcn_first': {'k_first_layer_wide': 6},
    'dcr_sdrf': {'k_imp_rows_count': 1, 'k_draw_partial': 1},
}
STORE_OR_ATOMIC = re.compile(r'(global|buffer|flat|scratch)_(store|atomic)\w*')


def _build_flags():
    m = re.search(r'^FLAGS="([^"]*)"', open(os.path.join(CSRC, 'build.sh')).read(), re.M)
    assert m, 'FLAGS not found in csrc/build.sh'
    return m.group(1).split()


def _instructions(lines):
    """(mnemonic, operands, comment) per line of a kernel's text; labels and directives give an empty mnemonic."""
    out = []
    for ln in lines:
        code, _, comment = ln.partition(';')
        parts = code.split(None, 1)
        mn = parts[0] if parts and not parts[0].startswith('.') and not parts[0].endswith(':') else ''
        out.append((mn, parts[1] if len(parts) > 1 and mn else '', comment))
    return out


@pytest.fixture(scope='module')
def kernel_asm(tmp_path_factory):
    """{kernel label: [(mnemonic, operands, comment), ...]} of the kernels in KERNELS, every instantiation."""
    if not (shutil.which(HIPCC) or os.path.exists(HIPCC)):
        pytest.skip('hipcc not found')
    tmp = tmp_path_factory.mktemp('ticket_asm')
    procs = {src: subprocess.Popen([HIPCC, *_build_flags(), '--cuda-device-only', '-S', f'{src}.hip', '-o', str(tmp / f'{src}.s')],
                                   cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for src in KERNELS}
    kernels = {}
    for src, p in procs.items():
        log = p.communicate(timeout=600)[0]
        assert p.returncode == 0, f'{src}.hip: {log[-2000:]}'
        label, body = None, []
        for ln in open(tmp / f'{src}.s').read().splitlines() + ['_Zend:']:
            m = re.match(r'(_Z\w+):', ln)
            if m:
                if label and any(k in label for k in KERNELS[src]):
                    kernels[label] = _instructions(body)
                label, body = m.group(1), []
            elif label:
                body.append(ln)
    return kernels


def _of(kernel_asm, name):
    return {lab: ins for lab, ins in kernel_asm.items() if re.search(r'\d' + name + r'(E|I)', lab)}


@pytest.mark.parametrize('name,count', [(k, c) for per in KERNELS.values() for k, c in per.items()])
def test_ticket_follows_a_store_drain(kernel_asm, name, count):
    found = _of(kernel_asm, name)
    assert len(found) == count, (name, sorted(found))
    for label, ins in found.items():
        markers = [i for i, (_, _, c) in enumerate(ins) if MARKER in c]
        assert markers, f'{label}: no last_arriver drain'
        # the drain is the wait itself, and the next vector-memory store or atomic is the ticket (a returning add).  A load may
        # come between: it publishes nothing (k_adam_multi reloads gridDim.x there from the dispatch packet)
        for i in markers:
            assert ins[i][0] == 's_waitcnt' and 'vmcnt(0)' in ins[i][1], (label, ins[i])
            nxt = next(((mn, ops) for mn, ops, _ in ins[i + 1:] if STORE_OR_ATOMIC.match(mn)), None)
            assert nxt and nxt[0].startswith('global_atomic_add') and re.search(r'\bsc0\b', nxt[1]), (label, nxt)
        # going back from every returning add to the previous store or atomic, a vmcnt(0) wait lies on the way
        adds = [i for i, (mn, ops, _) in enumerate(ins) if mn.startswith('global_atomic_add') and re.search(r'\bsc0\b', ops)]
        assert adds, f'{label}: no ticket'
        for i in adds:
            for mn, ops, _ in reversed(ins[:i]):
                if mn == 's_waitcnt' and 'vmcnt(0)' in ops:
                    break
                assert not STORE_OR_ATOMIC.match(mn), f'{label}: {mn} {ops} reaches the ticket undrained'
        # global_/buffer_ accesses only: a flat_ access waits on lgkmcnt too and may not be an sc1 load or store
        assert not [mn for mn, _, _ in ins if mn.startswith('flat_')], label


def test_no_hand_rolled_tickets():
    """One form of the hand-off: no workgroup-scope release fences (no release for another CU), no ticket outside the helper."""
    srcs = sorted(glob.glob(os.path.join(CSRC, '*.hip')) + glob.glob(os.path.join(CSRC, '*.h')))
    assert srcs
    tickets = []
    for path in srcs:
        text = open(path).read()
        assert not re.search(r'fence\s*\(\s*__ATOMIC_RELEASE\s*,\s*"workgroup"\s*\)', text), path
        tickets += [(os.path.basename(path), m.group(0)) for m in re.finditer(r'(atomicAdd|__hip_atomic_fetch_add)\s*\([^;]*\)\s*==[^;]*-\s*1', text)]
    assert len(tickets) == 1 and tickets[0][0] == 'dcr_internal.h', tickets
