"""Writes tests/golden/gier/ (a trimmed GIER tree: data only) and tests/golden/gier.npz (what the REFERENCE's GIER class
makes of it), for tests/test_gier_cpu.py.

    python tools/gen_golden_gier.py /path/to/reference

The tree: the first 24 records of splits/val_sess_3.json, the four id-list families restricted to them and renumbered, and
the two GIER vocabulary JSONs.  The reference's data/GIER/GIER.py is imported with stub modules for h5py, pandas,
matplotlib, cv2 and pycocotools (none is needed by the index code), as tools/gen_golden.py does for its shims.  Recorded per
data_mode in MODES: len(op_data), ReqId2PairId, the lengths of PairId2ReqId, the getReqIdx matrix and get_op_info per pair.
The test reads only the fixture and the tree."""
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, SESSION, PHASE = 24, 3, 'val'
MODES = ['full', 'shapeAlign', 'valid+global']
FAMILIES = ['Ids_L1Thr_0.06', 'shapeAlign', 'shapeAlignNonCrop', 'global']


def write_tree(ref, out):
    os.makedirs(os.path.join(out, 'splits'), exist_ok=True)
    os.makedirs(os.path.join(out, 'language'), exist_ok=True)
    src = os.path.join(ref, 'data', 'GIER', 'splits')
    with open(os.path.join(src, '%s_sess_%d.json' % (PHASE, SESSION))) as f:
        text = f.read()
    records = json.loads(text)[:N]                                     # (NaN fields survive: Python's json reads and writes them)
    with open(os.path.join(out, 'splits', '%s_sess_%d.json' % (PHASE, SESSION)), 'w') as f:
        json.dump(records, f)
    for fam in FAMILIES:
        with open(os.path.join(src, '%s_%s_sess_%d.json' % (PHASE, fam, SESSION))) as f:
            ids = [int(i) for i in json.load(f) if int(i) < N]         # the first N records keep their numbers
        with open(os.path.join(out, 'splits', '%s_%s_sess_%d.json' % (PHASE, fam, SESSION)), 'w') as f:
            json.dump(ids, f)
    for name in ('GIER_vocabs_sess_%d.json' % SESSION, 'GIER_operator_vocabs_sess_%d.json' % SESSION):
        with open(os.path.join(ref, 'data', 'language', name)) as f:
            vocab = json.load(f)
        with open(os.path.join(out, 'language', name), 'w') as f:
            json.dump(vocab, f)


def reference_class(ref):
    for name in ('h5py', 'pandas', 'cv2', 'matplotlib', 'matplotlib.pyplot', 'pycocotools', 'pycocotools.mask'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules['matplotlib'].use = lambda *a, **k: None
    sys.modules['matplotlib'].pyplot = sys.modules['matplotlib.pyplot']
    sys.modules['pycocotools'].mask = sys.modules['pycocotools.mask']
    sys.modules['pycocotools.mask'].decode = None
    sys.path.insert(0, ref)
    from data.GIER.GIER import GIER
    return GIER


def main(ref):
    tree = os.path.join(ROOT, 'tests', 'golden', 'gier')
    write_tree(ref, tree)
    GIER = reference_class(ref)
    out = {}
    for mode in MODES:
        g = GIER(tree, os.path.join(tree, 'language'), PHASE, mode, False, SESSION)
        key = mode.replace('+', '_')
        n_req = len(g.ReqId2PairId)
        out[key + '_len'] = np.array(len(g.op_data))
        out[key + '_req2pair'] = np.array([g.ReqId2PairId[r] for r in range(n_req)], np.int64)
        out[key + '_pair2req_len'] = np.array([len(g.PairId2ReqId[p]) for p in range(len(g.op_data))], np.int64)
        out[key + '_req_idx'] = np.stack([g.getReqIdx[r] for r in range(n_req)]).astype(np.int64)
        infos = [g.get_op_info(p) for p in range(len(g.op_data))]
        out[key + '_op_idx'] = np.array([i[0] for i in infos], np.int64)
        out[key + '_is_local'] = np.array([i[1] for i in infos], np.int64)
        out[key + '_mask_ids'] = np.array(json.dumps([{str(k): v for k, v in i[2].items()} for i in infos]))
        out[key + '_n_op_req'] = np.array(len(g.OpReqId2ReqId))
        out[key + '_n_imgs'] = np.array(len(g.getImgId))
    np.savez_compressed(os.path.join(ROOT, 'tests', 'golden', 'gier.npz'), **out)
    print({k: getattr(v, 'shape', None) for k, v in out.items()})


if __name__ == '__main__':
    main(sys.argv[1])
