"""CPU: the command-line surface of the HASQI quality targets - `--quality-targets` of the training entry point, `--score-quality` of
the inference one - and the unchanged behaviour of plain `--quality`."""
import pytest


def test_quality_targets_option_and_the_scorer_it_selects():
    from nele_gan_amd import quality, train_nele
    quality.clear_backends()
    ap = train_nele.build_parser()
    a = ap.parse_args(['--data', 'corpus'])
    assert a.quality is False and a.quality_targets == 'programs' and train_nele.quality_scorer_from_cli(ap, a) is None
    a = ap.parse_args(['--data', 'corpus', '--quality', '--quality-targets', 'hasqi'])        # needs no --pesq / --visqol
    sc = train_nele.quality_scorer_from_cli(ap, a)
    assert isinstance(sc, quality.HasqiScorer) and sc.on_device and sc.target_kind == 'hasqi' and sc.noise == 'utterance' and sc.seed == 0
    assert not getattr(quality.Scorer(), 'on_device', False)
    with pytest.raises(SystemExit):
        ap.parse_args(['--data', 'corpus', '--quality-targets', 'pesq'])
    with pytest.raises(ValueError):
        quality.HasqiScorer(noise='batch')


def test_plain_quality_without_the_programs_is_the_same_error(capsys):
    from nele_gan_amd import quality, train_nele
    quality.clear_backends()
    with pytest.raises(SystemExit) as e:
        train_nele.main(['--data', 'corpus', '--quality'])
    assert e.value.code == 2
    assert '--quality needs both programs: --pesq MODULE:FUNCTION and --visqol PROGRAM --visqol-model FILE' in capsys.readouterr().err
    with pytest.raises(SystemExit):                                                            # 'programs' spelled out is the same mode
        train_nele.main(['--data', 'corpus', '--quality', '--quality-targets', 'programs'])


def test_checkpoint_key_is_written_for_hasqi_targets_only():
    from nele_gan_amd import quality
    from nele_gan_amd.train_nele import GanTrainer
    tr = GanTrainer.__new__(GanTrainer)
    assert tr._quality_target_kind() == 'programs'
    tr.quality_scorer = quality.Scorer()
    assert tr._quality_target_kind() == 'programs'
    tr.quality_scorer = quality.HasqiScorer(noise=False)
    assert tr._quality_target_kind() == 'hasqi'


def test_the_learning_curve_line_gains_a_field_only_with_hasqi():
    from nele_gan_amd.train_nele import GanTrainer
    assert GanTrainer.validation_log_line(1.0, 2.0, 0.5, 3) == 'SIIB is 1.000, HASPI is 2.000, ESTOI is 0.500, PESQ is 0.000, VISQOL is 0.000, EPOCH:3 \n'
    assert GanTrainer.validation_log_line(1.0, 2.0, 0.5, 3, hasqi=0.25).endswith('VISQOL is 0.000, HASQI is 0.250, EPOCH:3 \n')


def test_score_quality_needs_score(capsys):
    from nele_gan_amd import inference
    with pytest.raises(SystemExit) as e:
        inference.main(['--clean', 'a', '--noise', 'b', '--score-quality'])
    assert e.value.code == 2 and '--score-quality needs --score' in capsys.readouterr().err


def test_utterance_ids_are_a_stable_function_of_the_key():
    from nele_gan_amd import quality
    ids = quality.utterance_ids(['a.wav', 'b.wav', ('room', 'x', 3, 'a.wav'), 'a.wav'])
    assert ids.dtype.name == 'int64' and ids[0] == ids[3] and len(set(ids.tolist())) == 3
    assert int(ids[0]) == -8216239911213052915                              # the same in every process (not hash())
