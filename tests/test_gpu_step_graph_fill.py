"""t2o_graph_memsets_to_kernels and its fill kernel (k_graph_fill, t2o_optim.hip): every memset node of a graph becomes a
kernel node that writes the same bytes in the same place of the order.  Linear graphs only; guard bytes around every fill
and every byte compared against the memset node's semantics on the host (step_cases.fill_bytes)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import step_cases as sc

pytestmark = pytest.mark.gpu

KERNEL_NODE, MEMSET_NODE = 0, 2                        # hipGraphNodeType


class MemsetParams(ctypes.Structure):                  # hipMemsetParams
    _fields_ = [('dst', ctypes.c_void_p), ('elementSize', ctypes.c_uint), ('height', ctypes.c_size_t), ('pitch', ctypes.c_size_t),
                ('value', ctypes.c_uint), ('width', ctypes.c_size_t)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def hip():
    lib = ctypes.CDLL('libamdhip64.so')
    P, Z, I, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint
    lib.hipMemsetAsync.argtypes = [P, I, Z, P]
    lib.hipMemsetD16Async.argtypes = [P, ctypes.c_ushort, Z, P]
    lib.hipMemsetD32Async.argtypes = [P, I, Z, P]
    lib.hipGraphCreate.argtypes = [ctypes.POINTER(P), U]
    lib.hipGraphAddMemsetNode.argtypes = [ctypes.POINTER(P), P, ctypes.POINTER(P), Z, ctypes.POINTER(MemsetParams)]
    lib.hipGraphGetNodes.argtypes = [P, ctypes.POINTER(P), ctypes.POINTER(Z)]
    lib.hipGraphNodeGetType.argtypes = [P, ctypes.POINTER(I)]
    lib.hipGraphNodeGetDependencies.argtypes = [P, ctypes.POINTER(P), ctypes.POINTER(Z)]
    lib.hipGraphNodeGetDependentNodes.argtypes = [P, ctypes.POINTER(P), ctypes.POINTER(Z)]
    lib.hipGraphMemsetNodeGetParams.argtypes = [P, ctypes.POINTER(MemsetParams)]
    lib.hipGraphInstantiate.argtypes = [ctypes.POINTER(P), P, P, P, Z]
    lib.hipGraphLaunch.argtypes = [P, P]
    lib.hipGraphExecDestroy.argtypes = [P]
    lib.hipGraphDestroy.argtypes = [P]
    return lib


def graph_nodes(hip, graph):
    n = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) == 0
    nodes = (ctypes.c_void_p * max(n.value, 1))()
    assert hip.hipGraphGetNodes(graph, nodes, ctypes.byref(n)) == 0
    return [nodes[k] for k in range(n.value)]


def node_types(hip, graph):
    types = []
    for node in graph_nodes(hip, graph):
        t = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(node, ctypes.byref(t)) == 0
        types.append(t.value)
    return types


def memset_nodes(hip, graph):
    """{element size: (number of dependencies, number of dependents)} of the graph's memset nodes."""
    found = {}
    for node, t in zip(graph_nodes(hip, graph), node_types(hip, graph)):
        if t != MEMSET_NODE:
            continue
        mp = MemsetParams()
        assert hip.hipGraphMemsetNodeGetParams(node, ctypes.byref(mp)) == 0
        nd, nt = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert hip.hipGraphNodeGetDependencies(node, None, ctypes.byref(nd)) == 0
        assert hip.hipGraphNodeGetDependentNodes(node, None, ctypes.byref(nt)) == 0
        assert mp.elementSize not in found
        found[mp.elementSize] = (nd.value, nt.value)
    return found


def test_captured_fills_first_last_two_byte_and_more_than_one_grid_pass(dev, hip):
    """One captured stream: a 2-byte memset (odd count, two different bytes) as the FIRST node, a kernel, a kernel, a byte
    memset of 2^20 + 777 bytes at an odd address (4096 workgroups x 256 threads cover 2^20: a second grid pass), a kernel,
    a kernel, and a 4-byte memset as the LAST node."""
    from t2onet_amd import graphs
    n16, nbig, n32 = 333, (1 << 20) + 777, 17
    a = torch.zeros(1024, dtype=torch.uint8, device=dev)
    b = torch.zeros(nbig + 128, dtype=torch.uint8, device=dev)
    c = torch.zeros(64, dtype=torch.int32, device=dev)
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g, capture_error_mode='thread_local'):
        st = torch.cuda.current_stream(dev).cuda_stream
        assert hip.hipMemsetD16Async(a.data_ptr() + 16, 0xA15C, n16, st) == 0
        a.add_(1)
        b.fill_(3)
        assert hip.hipMemsetAsync(b.data_ptr() + 33, 0x5A, nbig, st) == 0
        b.add_(1)
        c.fill_(9)
        assert hip.hipMemsetD32Async(c.data_ptr() + 4 * 8, 0x5EADBEEF, n32, st) == 0
    graph = ctypes.c_void_p(g.raw_cuda_graph())
    before = node_types(hip, graph)
    assert before.count(MEMSET_NODE) == 3
    # the 2-byte memset really is the graph's first node (no dependencies), the 4-byte one its last (no dependents), the
    # byte memset lies between two nodes -- checked on the captured graph, not assumed from the order of the calls
    assert memset_nodes(hip, graph) == {2: (0, 1), 1: (1, 1), 4: (1, 0)}
    assert graphs._harden(g) == 3
    after = node_types(hip, graph)
    assert MEMSET_NODE not in after and len(after) == len(before) and after.count(KERNEL_NODE) == before.count(KERNEL_NODE) + 3
    ea = sc.fill_bytes(np.full(1024, 0x11, dtype=np.uint8), 16, 0xA15C, 2, n16) + 1
    eb = sc.fill_bytes(np.full(nbig + 128, 3, dtype=np.uint8), 33, 0x5A, 1, nbig) + 1
    ec = np.full(64, 9, dtype=np.int32)
    ec[8:8 + n32] = 0x5EADBEEF
    for _ in range(3):
        a.fill_(0x11)
        b.fill_(0x77)
        c.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(a.cpu().numpy(), ea)
        assert np.array_equal(b.cpu().numpy(), eb)
        assert np.array_equal(c.cpu().numpy(), ec)


@pytest.mark.parametrize('elem', [1, 2, 4])
def test_two_dimensional_memset_nodes_keep_pitch_and_order(dev, hip, elem):
    """A hand-built chain of three memset nodes that overwrite one another: the whole body with a guard byte (1-D), then 5
    rows of 37 elements at a pitch of 64 elements, then 3 rows of 11 elements inside those.  After the rewrite: three kernel
    nodes, no memset node; launched three times.  The columns between width and pitch keep the guard byte, the bytes before
    and after the body are untouched, and the inner fill lies on top of the outer one."""
    from t2onet_amd import _lib
    pitch, rows, guard = 64 * elem, 5, 64
    body = rows * pitch
    buf = torch.full((guard + body + guard,), 0xCD, dtype=torch.uint8, device=dev)
    base = buf.data_ptr() + guard
    assert base % 4 == 0
    v1, v2 = 0x11223344, 0xA1B2C3D4
    fills = [(0, 0xEE, 1, body, 1, body), (0, v1, elem, 37, rows, pitch), (pitch + 5 * elem, v2, elem, 11, 3, pitch)]
    graph = ctypes.c_void_p()
    assert hip.hipGraphCreate(ctypes.byref(graph), 0) == 0
    prev = None
    for off, value, es, width, height, pt in fills:
        mp = MemsetParams(base + off, es, height, pt, value & ((1 << (8 * es)) - 1), width)
        node = ctypes.c_void_p()
        deps = (ctypes.c_void_p * 1)(prev) if prev is not None else None
        rc = hip.hipGraphAddMemsetNode(ctypes.byref(node), graph, deps, 0 if prev is None else 1, ctypes.byref(mp))
        assert rc == 0, 'hipGraphAddMemsetNode: %d' % rc
        prev = node.value
    assert node_types(hip, graph) == [MEMSET_NODE] * 3
    replaced = ctypes.c_int(-1)
    _lib.check(_lib.load().t2o_graph_memsets_to_kernels(graph, ctypes.byref(replaced)), 't2o_graph_memsets_to_kernels')
    assert replaced.value == 3
    assert node_types(hip, graph) == [KERNEL_NODE] * 3
    ex = ctypes.c_void_p()
    assert hip.hipGraphInstantiate(ctypes.byref(ex), graph, None, None, 0) == 0
    torch.cuda.synchronize()                                          # (the buffer's initial bytes are in place)
    side = torch.cuda.Stream(dev)
    for _ in range(3):
        assert hip.hipGraphLaunch(ex, side.cuda_stream) == 0
    torch.cuda.synchronize()
    expect = np.full(guard + body + guard, 0xCD, dtype=np.uint8)
    for off, value, es, width, height, pt in fills:
        sc.fill_bytes(expect, guard + off, value, es, width, height, pt)
    got = buf.cpu().numpy()
    assert hip.hipGraphExecDestroy(ex) == 0 and hip.hipGraphDestroy(graph) == 0
    assert np.array_equal(got, expect), np.flatnonzero(got != expect)[:8]
    body_rows = got[guard:guard + body].reshape(rows, pitch)
    assert (body_rows[:, 37 * elem:] == 0xEE).all() and (body_rows[2, 5 * elem:16 * elem] != body_rows[0, 5 * elem:16 * elem]).any()
