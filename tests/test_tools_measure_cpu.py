"""tools/_measure.py, the one measurement module of the tools/*_time.py family, checked without a device: the report's arithmetic, the
order in which ``interleaved`` warms and times its legs (fake timers), the summed-spreads rule at its boundary, the launch counter, the
bench.py comparison on stand-in trees, and every converted tool's imports, argument parsing and refusal to run without a GPU."""
import math
import os
import re
import subprocess
import sys
import types

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(REPO, 'tools')
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)

import _measure as M  # noqa: E402

CONVERTED = ('eval_epilogue_time', 'eval_label_time', 'validate_time', 'validate_label_time', 'weighted_loss_time', 'overlay_time',
             'confidence_time', 'ingest_time', 'frame_resize_time', 'batch_augment_time', 'voc_batch_augment_time', 'label_codec_time',
             'color_jitter_time', 'rotate_time', 'gaussian_blur_time')
ONLY_IN_MEASURE = ('region_ms', 'wall_ms', 'protocol_ms', 'host_ms', 'report', 'interleaved', 'bench_value', 'count_launches')


# ---- report
def test_report_medians_spreads_and_samples():
    lines = []
    med, spread = M.report(lines, 'the title', {'a': [3, 1, 2], 'b': [5, 5, 5]})
    assert med == {'a': 2, 'b': 5} and spread == {'a': 2, 'b': 0}
    assert lines[0] == 'the title' and len(lines) == 3
    assert lines[1].startswith('  a median 2.0000  min 1.0000  max 3.0000  spread 2.0000')
    assert lines[1].endswith('samples 3.0000 1.0000 2.0000') and lines[2].endswith('samples 5.0000 5.0000 5.0000')


def test_report_sizes_the_label_column_from_the_longest_label():
    long = 'x' * 80
    lines = []
    M.report(lines, 't', {long: [1.0], 'short': [2.0]})
    assert long in lines[1]
    assert lines[1].index(' median ') == lines[2].index(' median ')          # one column for both legs


def test_report_without_a_title_adds_no_title_line():
    lines = []
    M.report(lines, None, {'(a)': [1.0, 2.0]})
    assert lines == ['(a) median 1.5000  min 1.0000  max 2.0000  spread 1.0000   samples 1.0000 2.0000']


# ---- interleaved
def _fake_legs(log):
    def timer_of(tag):
        def timer(fn, reps):
            log.append((tag, fn.__name__, reps))
            return {'ta': 1.0, 'tb': 2.0}[tag]
        return timer

    def a():
        log.append('call a')

    def b():
        log.append('call b')
    return {'leg a': (timer_of('ta'), a, 7), 'leg b': (timer_of('tb'), b, 11)}


@pytest.mark.parametrize('warmup', [2, 0])
def test_interleaved_warms_every_leg_then_times_the_legs_in_turn(monkeypatch, warmup):
    log = []
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda: log.append('sync'))
    lines = []
    med, spread = M.interleaved(lines, 'group', _fake_legs(log), rounds=3, warmup=warmup)
    assert log == ['call a'] * warmup + ['call b'] * warmup + ['sync'] + [('ta', 'a', 7), ('tb', 'b', 11)] * 3
    assert med == {'leg a': 1.0, 'leg b': 2.0} and spread == {'leg a': 0.0, 'leg b': 0.0}
    assert lines[0] == 'group' and len(lines) == 3


# ---- the summed-spreads rule
def test_the_rule_at_its_boundary():
    spread = {'a': 0.25, 'b': 0.25}
    equal = {'a': 1.0, 'b': 1.5}                                        # b - a == spread[a] + spread[b], exactly
    above = {'a': 1.0, 'b': math.nextafter(1.5, 2.0)}                   # one ulp more
    assert above['b'] - above['a'] > 0.5 == equal['b'] - equal['a']
    assert not M.exceeds('b', 'a', equal, spread) and not M.exceeds('a', 'b', equal, spread)
    assert M.exceeds('b', 'a', above, spread) and not M.exceeds('a', 'b', above, spread)
    assert M.verdict('(b) - (a)', 'a', 'b', equal, spread) == '(b) - (a) = +0.5000 ms, summed spreads 0.5000: within'
    assert M.verdict('(b) - (a)', 'a', 'b', above, spread) == '(b) - (a) = +0.5000 ms, summed spreads 0.5000: beyond'
    assert M.verdict('(a) - (b)', 'b', 'a', above, spread).endswith('-0.5000 ms, summed spreads 0.5000: beyond')     # either direction


# ---- count_launches
def test_count_launches_counts_per_name_and_restores():
    calls = []
    lib = types.SimpleNamespace(hs_one=lambda *a: calls.append(('one', a)), hs_two=lambda *a: calls.append(('two', a)),
                                hs_other=lambda *a: calls.append(('other', a)))
    originals = dict(vars(lib))

    def fn():
        lib.hs_one(1)
        lib.hs_two(2, None)
        lib.hs_one(3)
        lib.hs_other()
    assert M.count_launches(lib, ('hs_one', 'hs_two'), fn) == {'hs_one': 2, 'hs_two': 1}
    assert calls == [('one', (1,)), ('two', (2, None)), ('one', (3,)), ('other', ())]          # the real entries still ran
    assert vars(lib) == originals
    weighted = M.count_launches(lib, ('hs_two',), lambda: (lib.hs_two(2, None), lib.hs_two(2, 'sums')),
                                weight=lambda name, args: 3 if args[1] is not None else 1)
    assert weighted == {'hs_two': 4}


def test_count_launches_restores_when_fn_raises():
    lib = types.SimpleNamespace(hs_one=lambda *a: None)
    original = lib.hs_one

    def fn():
        lib.hs_one()
        raise RuntimeError('the route failed')
    with pytest.raises(RuntimeError, match='the route failed'):
        M.count_launches(lib, ('hs_one',), fn)
    assert lib.hs_one is original


# ---- bench.py of two trees
def _tree(root, name, body):
    os.makedirs(root / name)
    (root / name / 'bench.py').write_text(body)
    return str(root / name)


def _bench_script(log, tag, value):
    return (f"import sys\nopen({str(log)!r}, 'a').write({tag!r} + ' ' + ' '.join(sys.argv[1:]) + '\\n')\n"
            f"print('starting\\n{{\"value\": 1.0}}\\n[log] noise\\n{{\"value\": {value}}}')\n")


def test_bench_value_reads_the_last_json_line(tmp_path):
    log = tmp_path / 'log.txt'
    assert M.bench_value(_tree(tmp_path, 'tree', _bench_script(log, 'tree', 12.5))) == 12.5
    assert log.read_text() == 'tree --gpus 1 --steps 200 --warmup 20\n'


def test_bench_value_raises_where_bench_fails(tmp_path):
    with pytest.raises(subprocess.CalledProcessError):
        M.bench_value(_tree(tmp_path, 'tree', 'import sys\nsys.exit(1)\n'))


def test_compare_bench_alternates_parent_and_this_tree(tmp_path, monkeypatch):
    log = tmp_path / 'log.txt'
    parent = _tree(tmp_path, 'parent', _bench_script(log, 'parent', 10.0))
    monkeypatch.setattr(M, 'REPO', _tree(tmp_path, 'this', _bench_script(log, 'this', 12.0)))
    lines = ['written before']
    assert M.compare_bench(lines, parent, rounds=2) is None
    assert [ln.split()[0] for ln in log.read_text().splitlines()] == ['parent', 'this', 'parent', 'this']
    assert lines == ['written before', 'bench.py --gpus 1 --steps 200 --warmup 20, fresh processes, alternating, 2 each; frames/s',
                     '  parent     median 10.00  min 10.00  max 10.00   samples 10.00 10.00',
                     '  this tree  median 12.00  min 12.00  max 12.00   samples 12.00 12.00']


def test_compare_bench_hands_back_the_error_that_stopped_it(tmp_path, monkeypatch):
    log = tmp_path / 'log.txt'
    failing_second_time = (f"import sys\nsys.exit(1) if open({str(log)!r}).read().count('parent') else None\n" + _bench_script(log, 'parent', 10.0))
    log.write_text('')
    parent = _tree(tmp_path, 'parent', failing_second_time)
    monkeypatch.setattr(M, 'REPO', _tree(tmp_path, 'this', _bench_script(log, 'this', 12.0)))
    lines = ['written before']
    error = M.compare_bench(lines, parent, rounds=3)
    assert isinstance(error, subprocess.CalledProcessError)
    assert [ln.split()[0] for ln in log.read_text().splitlines()] == ['parent', 'this']              # nothing ran after the failure
    assert lines[0] == 'written before' and lines[2].endswith('samples 10.00') and lines[3].endswith('samples 12.00')
    assert lines[4] == '  the comparison stopped early: CalledProcessError' and len(lines) == 5


def test_compare_bench_where_the_parent_fails_at_once(tmp_path, monkeypatch):
    parent = _tree(tmp_path, 'parent', 'import sys\nsys.exit(1)\n')
    monkeypatch.setattr(M, 'REPO', _tree(tmp_path, 'this', 'import sys\nsys.exit(1)\n'))
    lines = ['written before']
    error = M.compare_bench(lines, parent, rounds=2)
    assert isinstance(error, subprocess.CalledProcessError)
    assert lines[0] == 'written before' and lines[-1] == '  the comparison stopped early: CalledProcessError' and len(lines) == 3


def test_compare_bench_without_a_parent_tree_says_so():
    lines = []
    assert M.compare_bench(lines, None, rounds=3) is None
    assert lines == ['bench.py: no --parent-tree given, not compared in this run']


# ---- Lines, write_report, require_gpu
def test_lines_prints_as_it_appends(capsys):
    lines = M.Lines()
    lines.append('first')
    assert capsys.readouterr().out == 'first\n'
    lines.append('second')
    assert capsys.readouterr().out == 'second\n' and lines == ['first', 'second']


def test_write_report_creates_a_missing_directory(tmp_path):
    out = tmp_path / 'not' / 'there' / 'report.txt'
    M.write_report(['one', 'two'], str(out))
    assert out.read_text() == 'one\ntwo\n'


def test_require_gpu_fails_where_no_device_is_found(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(SystemExit, match='^some_time.py measures on the GPU: no device found$'):
        M.require_gpu('some_time.py')
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    M.require_gpu('some_time.py')


# ---- the converted tools
@pytest.mark.parametrize('tool', CONVERTED)
def test_tool_parses_its_arguments_and_refuses_to_run_without_a_gpu(tool, tmp_path):
    """``--help`` exits 0 (imports and argument parsing work).  With every device hidden from the child the tool exits non-zero with
    ``require_gpu``'s message before it has written a report."""
    script, out = os.path.join(TOOLS, tool + '.py'), tmp_path / 'report.txt'
    hidden = dict(os.environ, HIP_VISIBLE_DEVICES='-1', CUDA_VISIBLE_DEVICES='-1')
    pipes = dict(stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=str(tmp_path))
    helped = subprocess.Popen([sys.executable, script, '--help'], **pipes)
    refused = subprocess.Popen([sys.executable, script, '--out', str(out)], env=hidden, **pipes)
    try:
        help_text, help_err = helped.communicate(timeout=120)
        _, refusal = refused.communicate(timeout=120)
    finally:
        helped.kill()
        refused.kill()
    assert helped.returncode == 0, help_err
    assert '--out' in help_text and '--rounds' in help_text
    assert refused.returncode != 0
    assert refusal.strip().splitlines()[-1] == f'{tool}.py measures on the GPU: no device found'
    assert not out.exists()


def test_the_helpers_are_defined_once_and_no_tool_imports_another():
    defines = re.compile(r'^\s*def (%s)\b' % '|'.join(ONLY_IN_MEASURE), re.M)
    imports_a_tool = re.compile(r'^\s*(?:from\s+\w*_time\s+import|import\s+\w*_time\b)', re.M)
    names = sorted(n for n in os.listdir(TOOLS) if n.endswith('.py'))
    assert '_measure.py' in names and all(t + '.py' in names for t in CONVERTED)
    for name in names:
        text = open(os.path.join(TOOLS, name)).read()
        if name == '_measure.py':
            assert sorted(defines.findall(text)) == sorted(ONLY_IN_MEASURE)
        else:
            assert defines.findall(text) == [], name
        assert imports_a_tool.findall(text) == [], name
