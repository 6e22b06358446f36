"""The device data step on the GPU (t2o_image_io.hip), bit for bit against the host path it replaces: the batched 8-bit
resize + layout conversion (functional.resize_u8), its inverse for writing images (functional.to_u8_hwc), and the raw
datasets + collate_raw + device_batch against the default DataLoader batch."""
import os

import numpy as np
import pytest
import torch

from tests.test_image_io_cpu import OUTPUTS, SOURCES, edge_values, numpy_path, source_images

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def mixed():
    """The eight sources, three images each (random, all 0, all 255), as ONE batch at odd byte offsets (1, 2, 3 pad
    bytes in turn), and the numpy path's result per output size -- computed once, never modified."""
    images = [im for k, s in enumerate(SOURCES) for im in source_images(s, 11 + 97 * k)]
    pads = [1 + i % 3 for i in range(len(images))]
    want = {o: torch.from_numpy(np.stack([numpy_path(im, *o) for im in images])) for o in OUTPUTS}
    return images, pads, want


def _kernels(prof):
    from torch.autograd import DeviceType
    return [(e.key, e.count) for e in prof.key_averages() if e.device_type == DeviceType.CUDA]


@pytest.mark.parametrize('size', OUTPUTS)
def test_resize_mixed_batch_bit_exact(dev, mixed, size):
    import t2onet_amd.functional as T
    images, pads, want = mixed
    buffer, descs = T.pack_u8(images, pads=pads)
    assert len({int(d['offset']) % 4 for d in descs}) >= 3          # odd byte offsets: nothing is aligned
    n, (h, w) = len(images), size
    guard = 37
    big = torch.full((guard + n * 3 * h * w + guard,), float('nan'), device=dev)
    out = big[guard:guard + n * 3 * h * w].view(n, 3, h, w)
    got = T.resize_u8((buffer, descs), size, dev, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(got.cpu(), want[size])
    assert torch.isnan(big[:guard]).all() and torch.isnan(big[-guard:]).all()
    again = T.resize_u8(images, size, dev) if size[0] == size[1] else T.resize_u8((buffer, descs), size, dev)
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))


def test_resize_every_byte_value_and_absent_images(dev):
    import t2onet_amd.functional as T
    img = (np.arange(256 * 3).reshape(16, 16, 3) % 256).astype(np.uint8)
    got = T.resize_u8([img, None, img], 16, dev)
    ref = torch.from_numpy(numpy_path(img, 16, 16))
    assert torch.equal(got[0].cpu(), ref) and torch.equal(got[2].cpu(), ref)
    assert float(got[1].abs().sum()) == 0.0
    with pytest.raises(ValueError, match='outside'):
        buffer, descs = T.pack_u8([img])
        bad = descs.copy()
        bad['h'] = 17
        T.resize_u8((buffer, bad), 8, dev)


def test_resize_is_one_launch_and_one_upload(dev, mixed):
    import t2onet_amd.functional as T
    images, pads, want = mixed
    buffer, descs = T.pack_u8(images, pads=pads)
    T.resize_u8((buffer, descs), (13, 17), dev)
    torch.cuda.synchronize()
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = T.resize_u8((buffer, descs), (13, 17), dev)
        torch.cuda.synchronize()
    ks = _kernels(prof)
    print('resize_u8, %d images: %s' % (len(images), ks))
    assert torch.equal(out.cpu(), want[(13, 17)])
    kernels = [(k, c) for k, c in ks if not k.startswith('Memcpy')]
    copies = [(k, c) for k, c in ks if k.startswith('Memcpy')]
    assert len(kernels) == 1 and 'k_resize_u8_f32' in kernels[0][0] and kernels[0][1] == 1, ks
    assert len(copies) == 1 and copies[0][1] == 1 and 'DtoH' not in copies[0][0] and 'DtoD' not in copies[0][0], ks


def _inverse_case(shape, seed):
    n = int(np.prod(shape))
    v = np.random.default_rng(seed).random(n, dtype=np.float32)
    e = edge_values()
    v[:min(n, e.size)] = e[:min(n, e.size)]
    return torch.from_numpy(v.reshape(shape))


@pytest.mark.parametrize('shape', [(2, 3, 5, 7), (1, 3, 1, 1), (1, 3, 9, 64)])
def test_inverse_bit_exact(dev, shape):
    import t2onet_amd.functional as T
    cases = [_inverse_case(shape, 21)]
    if shape == (1, 3, 9, 64):                                 # every edge value (770 of them) fits here
        t = torch.from_numpy(np.resize(edge_values(), int(np.prod(shape))).reshape(shape).copy())
        cases.append(t)
    for t in cases:
        want = (t * 255).permute(0, 2, 3, 1).numpy().astype(np.uint8)
        got = T.to_u8_hwc(t.to(dev))
        assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
        assert np.array_equal(got.cpu().numpy(), want)
        for lead in (0, 1, 2, 3):                              # every alignment of the output; sentinels on both sides
            big = torch.full((lead + want.size + 9,), 201, dtype=torch.uint8, device=dev)
            T.to_u8_hwc(t.to(dev), out=big[lead:lead + want.size])
            host = big.cpu().numpy()
            assert np.array_equal(host[lead:lead + want.size].reshape(want.shape), want)
            assert (host[:lead] == 201).all() and (host[lead + want.size:] == 201).all()


def test_device_batch_equals_default_loader(dev, tmp_path):
    from t2onet_amd import data
    from tests import fivek_tree
    img_dir, anno_dir, act_dir, _ = fivek_tree.write_tree(str(tmp_path), n_train=4, n_val=2)
    ref = data.FiveKAct(img_dir, anno_dir, act_dir, 'train', 1, 16)
    raw = data.FiveKAct(img_dir, anno_dir, act_dir, 'train', 1, 16, raw=True)
    want = next(iter(torch.utils.data.DataLoader(ref, batch_size=4)))
    loader = torch.utils.data.DataLoader(raw, batch_size=4, collate_fn=data.collate_raw, pin_memory=True)
    got = data.device_batch(next(iter(loader)), 16, dev)
    assert len(got) == len(want) == 6
    zero_slots = 0
    for g, w in zip(got, want):
        if torch.is_tensor(w):
            assert g.is_cuda and g.dtype == w.dtype and g.shape == w.shape and g.is_contiguous()
            assert torch.equal(g.cpu(), w)
        else:
            assert list(g) == list(w)
    for b in range(4):
        n = int((want[3][b] > 2).sum())
        zero_slots += 5 - n
        assert float(got[1][b, n:5].abs().sum()) == 0.0 and float(got[1][b, 5].sum()) > 0
    assert zero_slots > 0
    # FiveK: the training form (pairs to a square) and the validation form (short side, a non-square image)
    want = next(iter(torch.utils.data.DataLoader(data.FiveK(img_dir, anno_dir, 'train', 1, 16), batch_size=3)))
    got = data.device_batch(data.collate_raw([data.FiveK(img_dir, anno_dir, 'train', 1, 16, raw=True)[i] for i in range(3)]), 16, dev)
    assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1]) and torch.equal(got[2].cpu(), want[2])
    val = data.FiveK(img_dir, anno_dir, 'val', 1, short_size=24)
    val_raw = data.FiveK(img_dir, anno_dir, 'val', 1, short_size=24, raw=True)
    for i in range(2):
        want = next(iter(torch.utils.data.DataLoader(torch.utils.data.Subset(val, [i]), batch_size=1)))
        got = data.device_batch(data.collate_raw([val_raw[i]]), device=dev, short_size=24)
        assert tuple(want[0].shape[2:]) in ((24, 36), (36, 24))
        assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1])
        assert torch.equal(got[2].cpu(), want[2]) and list(got[3]) == list(want[3])


def test_write_record_from_gpu_tensors_writes_the_same_bytes(dev, tmp_path):
    from t2onet_amd import plan_cli
    g = torch.Generator().manual_seed(3)
    x, y = torch.rand(1, 3, 19, 23, generator=g), torch.rand(1, 3, 19, 23, generator=g)
    imgs = [torch.rand(1, 3, 19, 23, generator=g) for _ in range(2)]
    imgs[1].view(-1)[:770] = torch.from_numpy(edge_values())
    seq = [('brightness', [0.5], 0.2), ('contrast', [0.25], 0.1)]
    assert np.array_equal(plan_cli.tensor2img(x.to(dev)), plan_cli.tensor2img(x))
    plan_cli.write_record(str(tmp_path / 'cpu'), 'train', 0, 'req', 0.3, [seq], [imgs], x, y)
    plan_cli.write_record(str(tmp_path / 'gpu'), 'train', 0, 'req', 0.3, [seq], [[t.to(dev) for t in imgs]], x.to(dev), y.to(dev))
    names = sorted(os.listdir(str(tmp_path / 'cpu' / 'train0')))
    assert names == sorted(os.listdir(str(tmp_path / 'gpu' / 'train0'))) and len(names) == 5
    for name in names:
        with open(str(tmp_path / 'cpu' / 'train0' / name), 'rb') as a, open(str(tmp_path / 'gpu' / 'train0' / name), 'rb') as b:
            assert a.read() == b.read(), name


def test_non_default_stream(dev, mixed):
    import t2onet_amd.functional as T
    images, pads, want = mixed
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        out = T.resize_u8(images, (8, 12), dev)
        back = T.to_u8_hwc(out)
    s.synchronize()
    assert torch.equal(out.cpu(), want[(8, 12)])
    assert np.array_equal(back.cpu().numpy(), (want[(8, 12)] * 255).permute(0, 2, 3, 1).numpy().astype(np.uint8))


def test_train_cli_device_resize_on_a_fivek_layout_tree(tmp_path):
    """train_cli --device_resize end to end: raw loaders (workers only decode), device_batch for the train batches and the
    short-side validation images."""
    from t2onet_amd import train_cli
    from tests import fivek_tree
    img_dir, anno_dir, act_dir, glove = fivek_tree.write_tree(str(tmp_path / 'data'), n_train=4, n_val=1)
    avg = train_cli.main(['--img_dir', img_dir, '--anno_dir', anno_dir, '--act_dir', act_dir, '--word2vec', glove,
                          '--batch_size', '4', '--img_size', '64', '--num_iters', '2', '--print_every', '2', '--device_resize',
                          '--checkpoint_every', '2', '--run_dir', str(tmp_path / 'run'), '--num_workers', '0'])
    st = avg['stats']
    assert st['train_iter'] == [2] and len(st['val_dist']) == 1 and 0 < st['best_val_dist'] < 1
